// extern "C" entry points declared in include/fhe_ring.h: context set-up and the transform launches.
#include <hip/hip_runtime.h>
#include <cstdlib>

#include <cstring>
#include <mutex>
#include <new>
#include <set>
#include <utility>

#include "../../include/fhe_ring.h"
#include "api_common.hpp"
#include "ctx.hpp"
#include "dispatch.hpp"
#include "ntt_kernels.hpp"
#include "ntt14w.hpp"

using fhe::u64;

namespace {
// validates (ctx, n) the way the reference would panic
int check_transform(const fhe_ctx *ctx, const void *a, size_t n, size_t batch) {
    if (!ctx || !is_pow2(n) || (!a && batch)) return FHE_ERR_INVALID;
    if (n == 1) return FHE_OK;
    int log_n = ilog2(n);
    if (log_n > ctx->s - 1) return FHE_ERR_NO_ROOT;
    if (log_n > ctx->log_cap) return FHE_ERR_UNSUPPORTED;
    return FHE_OK;
}

// Which policy serves a modulus, by `pm` = the common bit length of pseudo-Mersenne eligible moduli (anything else: Shoup).  The lists
// are what is instantiated:
template <class F>
int with_wave_policy(int pm, F &&f) { return fhe::with_policy<fhe::ArithDS, 60, 54, 55>(pm, f); }  // the wave-local transforms (ntt14w.hpp)
// The lazy forward butterflies of those kernels are proved for c <= DsLazy<B>::CMAX (arith.hpp).  That bound is the eligibility bound of
// ctx_build_host itself: a modulus that reaches ArithDS at one of the listed widths is inside the proof, anything else takes Shoup
// arithmetic as before, so no modulus needs a second set of butterflies.  A width added to the list without this holding does not compile.
template <int... Bs>
constexpr bool lazy_covers_eligible() { return (... && (fhe::DsLazy<Bs>::CMAX >= ((unsigned __int128)1 << (Bs - 33)))); }
static_assert(lazy_covers_eligible<60, 54, 55>(), "a pseudo-Mersenne eligible modulus outside the lazy butterflies' proof");
template <class F>
int with_gen_policy(int pm, F &&f) { return fhe::with_policy<fhe::ArithPM, 60, 54, 55>(pm, f); }  // the generic kernels from N = 2^10 up
// the fused ring product has no 55-bit instantiation: 55-bit moduli take its Shoup kernel
template <class F>
int with_mul_policy(int pm, F &&f) { return fhe::with_policy<fhe::ArithDS, 60, 54>(pm, f); }
// (55 bits: the reference's own parameter sets, scheme/fhew/examples/multi_key_uint8.rs:15-29, util/src/ring/rns.rs:373-386)

// the generic kernels' shape per ring size, LOG_N -> (LOG_E, PPW): 16 coefficients per thread from N = 128 up; small rings pack many
// polynomials into one 64..256-thread workgroup
struct GenShape { int log_e, ppw; };
constexpr GenShape GEN_SHAPE[14] = {{0, 0}, {1, 64}, {2, 64}, {3, 64}, {4, 64}, {3, 16}, {3, 16}, {4, 16}, {4, 16}, {4, 8}, {4, 4}, {4, 2}, {4, 1}, {4, 1}};

template <class A, int LOG_N>
int launch_gen(bool inverse, const fhe::ModDesc *descs, unsigned n_desc, u64 *a, size_t subs, hipStream_t st, fhe::NttIo io) {
    constexpr int LOG_E = GEN_SHAPE[LOG_N].log_e, PPW = GEN_SHAPE[LOG_N].ppw;
    using C = fhe::NttCfg<LOG_N, LOG_E, PPW>;
    // measured on MI355X (tools/ntt_lab.hip): staging through LDS wins for the forward stores, direct 16-byte loads win
    // for the inverse
    const unsigned grid = (unsigned)((subs + PPW - 1) / PPW);
    if (inverse)
        return fhe::launch<fhe::ntt_inv_kernel<A, LOG_N, LOG_E, PPW, false, true>>(grid, C::THREADS, C::LDS_BYTES, st, a, descs, n_desc, (unsigned)subs, 0, io);
    return fhe::launch<fhe::ntt_fwd_kernel<A, LOG_N, LOG_E, PPW, false, false>>(grid, C::THREADS, C::LDS_BYTES, st, a, descs, n_desc, (unsigned)subs, 0, io);
}
// Shoup arithmetic at every size N = 2 .. 2^13, the pseudo-Mersenne policies from 2^10 up
template <class A>
int dispatch_gen(bool inv, int log_n, const fhe::ModDesc *d, unsigned nd, u64 *a, size_t subs, hipStream_t st, fhe::NttIo io) {
    auto size = [&](auto ln) { return launch_gen<A, decltype(ln)::value>(inv, d, nd, a, subs, st, io); };
    if constexpr (std::is_same_v<A, fhe::ArithShoup>) return fhe::with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13>(log_n, size);
    else return fhe::with_int<10, 11, 12, 13>(log_n, size);
}

// N = 2^14 (and the 2^14 sub-transforms of larger rings): the register-resident, wave-local kernels of ntt14w.hpp, two
// workgroups per CU.  Both directions run the two-operand twiddles (measured, tools/ntt_lab2.hip, 4096 transforms at 60 bits:
// forward 0.274 ms with ArithDS against 0.300 with the 8-byte ones (ArithPM); inverse 0.296 against
// 0.320 since its first pass runs in diagonal form and nothing spills: ntt14w.hpp).
inline bool limb_major_disabled() { return fhe::opt(fhe::OPT_NO_LIMB_MAJOR) != 0; }       // lab switch (api_common.hpp)
inline bool wave_local_small_disabled() { return fhe::opt(fhe::OPT_NO_W12) != 0; }       // 2^12 / 2^13 on the generic kernels
// a launch of the two-workgroups-per-CU kernels spans several generations of workgroups from this size on
inline size_t several_generations() { return size_t(8) * (size_t)fhe::current_cu_count(); }
template <class... P>
inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) % 16) == 0; }
// grid of a wave-local launch over `subs` blocks of `polys` polynomials.  Several moduli: modulus-major dispatch order (ntt14w.hpp,
// sub_of_block) -- only launches of several generations of workgroups: when the whole launch is resident at once the order is
// irrelevant, and measured 3 % slower at cfg4 batch 8
inline dim3 grid14(unsigned nd, size_t polys, size_t subs) {
    const bool by_mod = nd > 1 && nd <= 65535 && polys % nd == 0 && subs >= several_generations() && !limb_major_disabled();
    return by_mod ? dim3((unsigned)(subs / nd), nd) : dim3((unsigned)subs);
}
// workgroup and LDS size of a wave-local kernel follow from R0 (ntt14w.hpp: pass 0 has R0 layers, 2^R0 waves; N = 2^(11 + R0))
template <auto K, int R0>
int launch_w14(const fhe::ModDesc *d, unsigned nd, u64 *a, size_t subs, int pb, hipStream_t st, fhe::NttIo io) {
    return fhe::launch<K>(grid14(nd, subs >> pb, subs), fhe::w14::threads<R0>(), fhe::w14::lds_bytes<R0>(), st, a, d, nd, (unsigned)subs, pb, io);
}
template <class A, int R0>
int launch14(bool inv, const fhe::ModDesc *d, unsigned nd, u64 *a, size_t subs, int pb, hipStream_t st, fhe::NttIo io) {
    // every polynomial is read and written 16 bytes per lane (ntt14w.hpp); since the pass-0 side deals coefficient pairs that
    // includes the source of an out-of-place forward at 2^12 .. 2^14
    if (!aligned16(a, io.mul, io.dst2)) return FHE_ERR_INVALID;
    if constexpr (R0 <= 3) {
        if (!inv && !aligned16(io.src, io.src2, io.src3, io.src4)) return FHE_ERR_INVALID;
    }
    return fhe::with_bool(pb != 0, [&](auto pfx) {
        constexpr bool PFX = decltype(pfx)::value;
        if (!inv) return launch_w14<fhe::ntt14w_fwd_kernel<A, PFX, R0>, R0>(d, nd, a, subs, pb, st, io);
        return fhe::with_bool(io.mul != nullptr, [&](auto mul) {
            return launch_w14<fhe::ntt14w_inv_kernel<A, PFX, decltype(mul)::value, R0>, R0>(d, nd, a, subs, pb, st, io);
        });
    });
}

// the fused ring product (ntt14w_mul_kernel): a <- inverse(forward(a) (.) io.mul), 2^13 .. 2^15
template <class A, int R0>
int launch_mul14(const fhe::ModDesc *d, unsigned nd, u64 *a, size_t subs, hipStream_t st, fhe::NttIo io) {
    if (!aligned16(a, io.mul)) return FHE_ERR_INVALID;  // 16 bytes per lane on both sides (ntt14w.hpp)
    return launch_w14<fhe::ntt14w_mul_kernel<A, R0>, R0>(d, nd, a, subs, 0, st, io);
}

int sub_transform(bool inv, const fhe::ModDesc *d, unsigned nd, u64 *a, int log_n, size_t subs, int pb, int pm, hipStream_t st, fhe::NttIo io) {
    if (pb && log_n != 14) return FHE_ERR_UNSUPPORTED;
    // Wave-local form (ntt14w.hpp), R0 = log_n - 11.  2^15: whole rings in one pass over HBM, one workgroup of 1024 threads per CU.
    // 2^12 / 2^13 (two / four waves, each owning a 2^11 block; eight / four workgroups per CU): at 60 bits forward 3.3 -> 4.0 and
    // 2.8 -> 4.1 TB/s, inverse 2.9 -> 4.2 and 2.5 -> 3.9
    if (log_n == 14 || log_n == 15 || ((log_n == 12 || log_n == 13) && !wave_local_small_disabled()))
        return with_wave_policy(pm, [&](auto pol) {
            using A = typename decltype(pol)::type;
            return fhe::with_int<1, 2, 3, 4>(log_n - 11, [&](auto r0) { return launch14<A, decltype(r0)::value>(inv, d, nd, a, subs, pb, st, io); });
        });
    return with_gen_policy(log_n < 10 ? 0 : pm, [&](auto pol) {  // (below 2^10: Shoup arithmetic only)
        return dispatch_gen<typename decltype(pol)::type>(inv, log_n, d, nd, a, subs, st, io);
    });
}
int sub_fwd(const fhe::ModDesc *d, unsigned nd, u64 *a, int log_n, size_t subs, int pb, int pm, hipStream_t st, fhe::NttIo io) {
    return sub_transform(false, d, nd, a, log_n, subs, pb, pm, st, io);
}
int sub_inv(const fhe::ModDesc *d, unsigned nd, u64 *a, int log_n, size_t subs, int pb, int pm, hipStream_t st, fhe::NttIo io) {
    return sub_transform(true, d, nd, a, log_n, subs, pb, pm, st, io);
}

}  // namespace

namespace fhe {

// rings above 2^14 do not fit one workgroup's LDS: one radix-2^pb pass over HBM + 2^pb sub-transforms of 2^14.
// io counts POLYNOMIALS; the sub-transform launches take it in 2^14 blocks.
int ntt_fwd_multi(const ModDesc *descs, unsigned n_desc, u64 *a, int log_n, size_t batch, hipStream_t st, int pm, NttIo io) {
    if (io.mul) return FHE_ERR_INVALID;  // the pointwise multiplier belongs to the inverse
    if (log_n <= 15) return sub_fwd(descs, n_desc, a, log_n, batch, 0, pm, st, io);
    if (io.src_group) return FHE_ERR_UNSUPPORTED;  // several sources: single-pass rings only (callers fall back to one launch each)
    const int pb = log_n - 14;
    const size_t cols = batch << 14;
    // the opening pass reads the source, everything after it runs in place
    const int rc = with_int<1, 2, 3>(pb, [&](auto p) {
        return launch<ntt_big_fwd_pass<decltype(p)::value>>(grid_for(cols), 256, 0, st, a, descs, n_desc, (unsigned)batch, log_n, io.src, io.src_mod);
    });
    if (rc != FHE_OK) return rc;
    return sub_fwd(descs, n_desc, a, 14, batch << pb, pb, pm, st, NttIo());
}

int ntt_inv_multi(const ModDesc *descs, unsigned n_desc, u64 *a, int log_n, size_t batch, hipStream_t st, int pm, NttIo io) {
    if (io.src_group) return FHE_ERR_INVALID;
    if (log_n <= 15) return sub_inv(descs, n_desc, a, log_n, batch, 0, pm, st, io);
    const int pb = log_n - 14;
    NttIo sub_io = io;  // polynomial counts -> 2^14 block counts
    sub_io.src_mod = io.src_mod << pb; sub_io.mul_div = io.mul_div << pb; sub_io.mul_period = io.mul_period << pb;
    int rc = sub_inv(descs, n_desc, a, 14, batch << pb, pb, pm, st, sub_io);
    if (rc != FHE_OK) return rc;
    const size_t cols = batch << 14;
    return with_int<1, 2, 3>(pb, [&](auto p) {
        return launch<ntt_big_inv_pass<decltype(p)::value>>(grid_for(cols), 256, 0, st, a, descs, n_desc, (unsigned)batch, log_n);
    });
}

// N = 2^15 with the outermost layer left to the caller (rns_kernels.hpp, the edge kernels of the key switch): what remains of
// every polynomial are two independent 2^14 sub-transforms -- the two-workgroups-per-CU kernel instead of the one-per-CU 2^15 one.
// Forward: the caller has applied layer 0; inverse: the caller applies layer 0 and n^-1.  io counts polynomials.
int ntt_fwd_inner15(const ModDesc *descs, unsigned n_desc, u64 *a, size_t batch, hipStream_t st, int pm, NttIo io) {
    if (io.mul) return FHE_ERR_INVALID;
    io.src_mod <<= 1;
    return sub_fwd(descs, n_desc, a, 14, batch << 1, 1, pm, st, io);
}
int ntt_inv_inner15(const ModDesc *descs, unsigned n_desc, u64 *a, size_t batch, hipStream_t st, int pm, NttIo io) {
    io.src_mod <<= 1; io.mul_div <<= 1; io.mul_period <<= 1;
    return sub_inv(descs, n_desc, a, 14, batch << 1, 1, pm, st, io);
}

// a[s] <- inverse(forward(a[s]) (.) io.mul[..]) in one launch where a fused kernel exists (2^13 .. 2^15), else forward + inverse
// with the product on the inverse's load.  io.mul as for ntt_inv_multi; io.src must be null.
int ntt_mul_multi(const ModDesc *descs, unsigned n_desc, u64 *a, int log_n, size_t batch, hipStream_t st, int pm, NttIo io) {
    if (!io.mul || io.src) return FHE_ERR_INVALID;
    const bool off = fhe::opt(fhe::OPT_NO_FUSED_MUL) != 0;  // lab switch (api_common.hpp)
    if (log_n >= 13 && log_n <= 15 && !off)
        return with_mul_policy(pm, [&](auto pol) {
            using A = typename decltype(pol)::type;
            return with_int<2, 3, 4>(log_n - 11, [&](auto r0) { return launch_mul14<A, decltype(r0)::value>(descs, n_desc, a, batch, st, io); });
        });
    int rc = ntt_fwd_multi(descs, n_desc, a, log_n, batch, st, pm);
    return rc != FHE_OK ? rc : ntt_inv_multi(descs, n_desc, a, log_n, batch, st, pm, io);
}

int ntt_fwd_device(const fhe_ctx *c, u64 *a, int log_n, size_t batch, hipStream_t st) { return ntt_fwd_multi(c->d_desc, 1, a, log_n, batch, st, c->pm_b); }
int ntt_inv_device(const fhe_ctx *c, u64 *a, int log_n, size_t batch, hipStream_t st) { return ntt_inv_multi(c->d_desc, 1, a, log_n, batch, st, c->pm_b); }

int ctx_build_host(uint64_t q, fhe_ctx *c) {
    if (q < 3) return FHE_ERR_INVALID;
    if (!is_prime_u64(q)) return FHE_ERR_NOT_PRIME;
    if (q >> 62) return FHE_ERR_UNSUPPORTED;  // lazy [0, 4q) arithmetic needs q < 2^62
    c->q = q;
    c->s = __builtin_ctzll(q - 1);
    c->g = smallest_nonresidue(q);
    if (c->g == 0) return FHE_ERR_INVALID;  // q = 3: `Zq::generator` finds nothing in 1..q-1 and unwraps None (zq.rs:99-105)
    c->omega = powmod(c->g, (q - 1) >> c->s, q);
    // the reference table has 2^(s-1) entries, entry j = omega^bitrev_{s-1}(j).  Bit-reversed tables are
    // prefix-nested, so the first 2^k entries equal psi^bitrev_k(j) with psi = omega^(2^(s-1-k)).
    c->log_cap = c->s - 1 < MAX_LOG_N ? c->s - 1 : MAX_LOG_N;
    const size_t cap = size_t(1) << c->log_cap;
    const u64 psi = powmod(c->omega, u64(1) << (c->s - 1 - c->log_cap), q);
    const u64 psi_inv = invmod(psi, q);
    std::vector<uint64_t> pw(cap), pwi(cap);
    uint64_t x = 1, y = 1;
    for (size_t i = 0; i < cap; ++i) {
        pw[i] = x; pwi[i] = y;
        x = mulmod(x, psi, q); y = mulmod(y, psi_inv, q);
    }
    c->tw.resize(cap); c->twi.resize(cap);
    for (size_t j = 0; j < cap; ++j) {
        size_t r = bitrev((unsigned)j, c->log_cap);
        c->tw[j] = pw[r]; c->twi[j] = pwi[r];
    }
    for (int k = 0; k < 32; ++k) {
        uint64_t n = (uint64_t(1) << k) % q;
        c->ninv[k] = n ? invmod(n, q) : 0;
        c->ninv_s[k] = shoup(c->ninv[k], q);
        c->ninv_w[k] = (n && c->twi.size() > 1) ? mulmod(c->ninv[k], c->twi[1], q) : 0;
        c->ninv_w_s[k] = shoup(c->ninv_w[k], q);
    }
    int nbits = 64 - __builtin_clzll(q);
    // pseudo-Mersenne eligibility (arith.hpp): q = 2^b - c with 33 <= b <= 60 and c <= 2^(b-33)
    c->pm_b = 0; c->pm_c = 0;
    if (nbits >= 34 && nbits <= 60) {
        const uint64_t cc = (uint64_t(1) << nbits) - q;
        if (cc <= (uint64_t(1) << (nbits - 33))) { c->pm_b = nbits; c->pm_c = (unsigned)cc; }
    }
    c->barrett = fhe::make_barrett(q);
    return FHE_OK;
}

}  // namespace fhe

extern "C" {

const char *fhe_version(void) { return "learn-fhe_amd 0.1 (gfx950)"; }
int fhe_last_hip_error(void) { return g_last_hip; }

// hand the library's cached stream-ordered scratch (api_common.hpp: one private pool per device) back to the driver
int fhe_trim(void) {
    int rc = FHE_OK;
    std::lock_guard<std::mutex> lock(fhe::pool_mutex());
    for (int dev = 0; dev < fhe::MAX_DEVICES; ++dev)
        if (fhe::g_pools[dev] && hipMemPoolTrimTo(fhe::g_pools[dev], 0) != hipSuccess) rc = FHE_ERR_HIP;
    return rc;
}

// lab switches (api_common.hpp): name without the FHE_RING_ prefix, upper or lower case
int fhe_set_option(const char *name, long value) {
    if (!name) return FHE_ERR_INVALID;
    for (int i = 0; i < fhe::OPT_COUNT; ++i) {
        const char *a = name, *b = fhe::OPT_NAMES[i];
        while (*a && *b && (*a == *b || *a - 32 == *b)) { ++a; ++b; }
        if (!*a && !*b) {
            if (!fhe::opt_value_ok(i, value)) return FHE_ERR_INVALID;
            fhe::options().v[i].store(value, std::memory_order_relaxed);
            return FHE_OK;
        }
    }
    return FHE_ERR_INVALID;
}

int fhe_is_prime(uint64_t q) { return fhe::is_prime_u64(q) ? 1 : 0; }

int fhe_two_adic_primes(int bits, int log_n, int count, uint64_t *out) {
    if (!out || bits <= log_n || bits > 63 || log_n < 0 || count < 0) return 0;
    uint64_t lo = 1ull << (bits - log_n - 1), hi = 1ull << (bits - log_n);
    int found = 0;
    for (uint64_t k = hi - 1; k >= lo && found < count; --k) {
        uint64_t c = (k << log_n) + 1;
        if (fhe::is_prime_u64(c)) out[found++] = c;
    }
    return found;
}

int fhe_ctx_create(uint64_t q, int device, fhe_ctx **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    fhe_ctx *c = new (std::nothrow) fhe_ctx();
    if (!c) return FHE_ERR_INVALID;
    int rc = fhe::ctx_build_host(q, c);
    if (rc != FHE_OK) { delete c; return rc; }
    c->device = device;
    if (device >= 0) {
        DeviceGuard guard(device);
        if (!guard.ok) { delete c; return FHE_ERR_HIP; }
        const size_t cap = c->tw.size();
        std::vector<fhe::TwPair> pf(cap), pi(cap);
        for (size_t j = 0; j < cap; ++j) {
            pf[j] = {c->tw[j], fhe::shoup(c->tw[j], q)};
            pi[j] = {c->twi[j], fhe::shoup(c->twi[j], q)};
        }
        hipError_t e = hipMalloc(&c->d_tw, cap * sizeof(fhe::TwPair));
        if (e == hipSuccess) e = hipMalloc(&c->d_twi, cap * sizeof(fhe::TwPair));
        if (e == hipSuccess) e = hipMemcpy(c->d_tw, pf.data(), cap * sizeof(fhe::TwPair), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(c->d_twi, pi.data(), cap * sizeof(fhe::TwPair), hipMemcpyHostToDevice);
        if (e == hipSuccess && c->pm_b) {
            // twiddles in the 8-byte form the pseudo-Mersenne policy loads: {wl, wh}, w = wl + wh 2^(b-31) (arith.hpp PmRaw)
            const int b = c->pm_b;
            std::vector<uint64_t> lf(cap), li(cap);
            auto pack = [b](uint64_t w) { return ((w >> (b - 31)) << 32) | (w & ((uint64_t(1) << (b - 31)) - 1)); };
            for (size_t j = 0; j < cap; ++j) { lf[j] = pack(c->tw[j]); li[j] = pack(c->twi[j]); }
            e = hipMalloc((void **)&c->d_tww, 2 * cap * sizeof(uint64_t));
            c->d_twwi = c->d_tww + cap;
            if (e == hipSuccess) e = hipMemcpy(c->d_tww, lf.data(), cap * sizeof(uint64_t), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(c->d_twwi, li.data(), cap * sizeof(uint64_t), hipMemcpyHostToDevice);
        }
        if (e == hipSuccess && c->pm_b) {
            // ... and in the 16-byte two-operand form {a0, a1, b0, b1} of ArithDS (w and w 2^32 mod q, each split at b - 31 bits)
            const int b = c->pm_b;
            std::vector<uint4> df(cap), di(cap);
            auto split = [b, q](uint64_t w) {
                const uint64_t w1 = (uint64_t)((((unsigned __int128)w) << 32) % q), lo = (uint64_t(1) << (b - 31)) - 1;
                return uint4{(unsigned)(w & lo), (unsigned)(w >> (b - 31)), (unsigned)(w1 & lo), (unsigned)(w1 >> (b - 31))};
            };
            for (size_t j = 0; j < cap; ++j) { df[j] = split(c->tw[j]); di[j] = split(c->twi[j]); }
            for (int k = 0; k < 20; ++k) { c->h_desc.ds_ninv[k] = split(c->ninv[k]); c->h_desc.ds_ninv_w[k] = split(c->ninv_w[k]); }
            c->h_desc.ds_one = split(1);
            e = hipMalloc((void **)&c->d_twd, 2 * cap * sizeof(uint4));
            c->d_twdi = c->d_twd + cap;
            if (e == hipSuccess) e = hipMemcpy(c->d_twd, df.data(), cap * sizeof(uint4), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(c->d_twdi, di.data(), cap * sizeof(uint4), hipMemcpyHostToDevice);
            // diagonal multipliers of the inverse's first pass (ntt14w.hpp): twd3i[(p - 1) stride + blk] = twi[4 blk]^p, p = 1..7
            if (e == hipSuccess && cap >= 8) {
                const size_t stride = cap / 4;
                std::vector<uint4> d3(7 * stride, uint4{0, 0, 0, 0});
                for (size_t blk = 1; blk < stride; ++blk) {
                    const uint64_t th = c->twi[4 * blk];
                    uint64_t pw = th;
                    for (int p = 0; p < 7; ++p) { d3[p * stride + blk] = split(pw); pw = fhe::mulmod(pw, th, q); }
                }
                e = hipMalloc((void **)&c->d_twd3i, d3.size() * sizeof(uint4));
                if (e == hipSuccess) e = hipMemcpy(c->d_twd3i, d3.data(), d3.size() * sizeof(uint4), hipMemcpyHostToDevice);
                c->h_desc.twd3i = c->d_twd3i; c->h_desc.twd3_stride = (unsigned)stride;
            }
        }
        c->h_desc.tww = c->d_tww;
        c->h_desc.twwi = c->d_twwi;
        c->h_desc.twd = c->d_twd;
        c->h_desc.twdi = c->d_twdi;
        c->h_desc.ds_pow = c->pm_b ? 1u << (c->pm_b - 31) : 0;
        c->h_desc.pm_b = c->pm_b;
        c->h_desc.pm_c = c->pm_c;
        c->h_desc.q = q;
        c->h_desc.tw = c->d_tw;
        c->h_desc.twi = c->d_twi;
        for (int k = 0; k < 20; ++k) {
            c->h_desc.ninv[k] = c->ninv[k]; c->h_desc.ninv_s[k] = c->ninv_s[k];
            c->h_desc.ninv_w[k] = c->ninv_w[k]; c->h_desc.ninv_w_s[k] = c->ninv_w_s[k];
        }
        c->h_desc.one_s = fhe::shoup(1, q);
        c->h_desc.bar_mu = c->barrett.mu; c->h_desc.bar_sh1 = c->barrett.sh1; c->h_desc.bar_sh2 = c->barrett.sh2;
        if (e == hipSuccess) e = hipMalloc(&c->d_desc, sizeof(fhe::ModDesc));
        if (e == hipSuccess) e = hipMemcpy(c->d_desc, &c->h_desc, sizeof(fhe::ModDesc), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            g_last_hip = (int)e;
            fhe_ctx_destroy(c);
            return FHE_ERR_HIP;
        }
    }
    *out = c;
    return FHE_OK;
}

void fhe_ctx_destroy(fhe_ctx *c) {
    if (!c) return;
    if (c->device >= 0) {
        DeviceGuard guard(c->device);
        if (c->d_tw) (void)hipFree(c->d_tw);
        if (c->d_twi) (void)hipFree(c->d_twi);
        if (c->d_desc) (void)hipFree(c->d_desc);
        if (c->d_tww) (void)hipFree(c->d_tww);
        if (c->d_twd) (void)hipFree(c->d_twd);
        if (c->d_twd3i) (void)hipFree(c->d_twd3i);
    }
    delete c;
}

int fhe_ctx_info(const fhe_ctx *c, uint64_t *q, int *s, uint64_t *g, uint64_t *omega) {
    if (!c) return FHE_ERR_INVALID;
    if (q) *q = c->q;
    if (s) *s = c->s;
    if (g) *g = c->g;
    if (omega) *omega = c->omega;
    return FHE_OK;
}

int fhe_ctx_twiddles(const fhe_ctx *c, int inverse, uint64_t *out, size_t count) {
    if (!c || !out) return FHE_ERR_INVALID;
    const auto &t = inverse ? c->twi : c->tw;
    if (count > t.size()) return FHE_ERR_UNSUPPORTED;
    std::memcpy(out, t.data(), count * sizeof(uint64_t));
    return FHE_OK;
}

static int transform_entry(const fhe_ctx *ctx, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream, bool inverse) {
    int rc = check_transform(ctx, a, n, batch);
    if (rc != FHE_OK) return rc;
    if (ctx->device < 0) return FHE_ERR_NO_DEVICE;
    if (n == 1 || batch == 0) return FHE_OK;
    if (batch > 0xffffffffull) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return FHE_ERR_HIP;
    Mirror m(a, n * batch, mem, true, st);
    if (m.rc != FHE_OK) return m.rc;
    rc = inverse ? fhe::ntt_inv_device(ctx, m.d, ilog2(n), batch, st) : fhe::ntt_fwd_device(ctx, m.d, ilog2(n), batch, st);
    if (rc != FHE_OK) return rc;
    return m.sync_out(st);
}

int fhe_ntt_fwd(const fhe_ctx *ctx, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream) {
    return transform_entry(ctx, a, n, batch, mem, stream, false);
}

int fhe_ntt_inv(const fhe_ctx *ctx, uint64_t *a, size_t n, size_t batch, fhe_mem mem, void *stream) {
    return transform_entry(ctx, a, n, batch, mem, stream, true);
}

static int launch_pointwise(const fhe_ctx *ctx, u64 *a, const u64 *b, size_t len, hipStream_t st) {
    return fhe::launch<fhe::pointwise_mul_kernel>(grid_for(len, 4096), 256, 0, st, a, b, len, ctx->barrett);
}

int fhe_pointwise_mul(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t len, fhe_mem mem, void *stream) {
    if (!ctx || ((!a || !b) && len)) return FHE_ERR_INVALID;
    if (ctx->device < 0) return FHE_ERR_NO_DEVICE;
    if (len == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return FHE_ERR_HIP;
    Mirror ma(a, len, mem, true, st), mb(b, len, mem, true, st);
    if (ma.rc != FHE_OK || mb.rc != FHE_OK) return FHE_ERR_HIP;
    int rc = launch_pointwise(ctx, ma.d, mb.d, len, st);
    if (rc != FHE_OK) return rc;
    return ma.sync_out(st);
}

namespace {
int rq_elementwise(uint64_t q, const void *a, const void *b, uint64_t *out, size_t len, int op, uint64_t scalar, fhe_mem mem, void *stream) {
    PtrDeviceGuard pguard(out, mem);
    if (!pguard.ok) return FHE_ERR_HIP;
    if (q < 2 || (q >> 62) || ((!a || !out || (op < 2 && !b)) && len) || (op == 3 && scalar >= q)) return FHE_ERR_INVALID;
    if (len == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    Mirror ma(a, len, mem, true, st), mb(op < 2 ? b : nullptr, op < 2 ? len : 0, mem, true, st), mo(out, len, mem, false, st);
    if (ma.rc | mb.rc | mo.rc) return FHE_ERR_HIP;
    FHE_TRY(fhe::launch<fhe::rq_elementwise_kernel>(grid_for(len), 256, 0, st, (const u64 *)ma.d, (const u64 *)mb.d, mo.d, len, op, (u64)scalar,
                                                     fhe::make_barrett(q)));
    return mo.sync_out(st);
}
}  // namespace

int fhe_rq_add(uint64_t q, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t len, fhe_mem mem, void *stream) {
    return rq_elementwise(q, a, b, out, len, 0, 0, mem, stream);
}
int fhe_rq_sub(uint64_t q, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t len, fhe_mem mem, void *stream) {
    return rq_elementwise(q, a, b, out, len, 1, 0, mem, stream);
}
int fhe_rq_neg(uint64_t q, const uint64_t *a, uint64_t *out, size_t len, fhe_mem mem, void *stream) {
    return rq_elementwise(q, a, nullptr, out, len, 2, 0, mem, stream);
}
int fhe_rq_scalar_mul(uint64_t q, const uint64_t *a, uint64_t scalar, uint64_t *out, size_t len, fhe_mem mem, void *stream) {
    return rq_elementwise(q, a, nullptr, out, len, 3, scalar, mem, stream);
}
int fhe_rq_from_i64(uint64_t q, const int64_t *in, uint64_t *out, size_t len, fhe_mem mem, void *stream) {
    return rq_elementwise(q, in, nullptr, out, len, 4, 0, mem, stream);
}

int fhe_ntt_mul(const fhe_ctx *ctx, uint64_t *a, const uint64_t *b, size_t n, size_t batch, fhe_mem mem,
                void *stream) {
    int rc = check_transform(ctx, a, n, batch);
    if (rc != FHE_OK) return rc;
    if (!b && batch) return FHE_ERR_INVALID;
    if (ctx->device < 0) return FHE_ERR_NO_DEVICE;
    if (batch == 0) return FHE_OK;
    if (batch > 0xffffffffull) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t count = n * batch;
    const int log_n = ilog2(n);
    Mirror ma(a, count, mem, true, st);
    if (ma.rc != FHE_OK) return ma.rc;
    // util/src/ring/fft/zq.rs:14-19 in three launches and 56 N bytes of HBM traffic instead of the reference's shape (copy of b,
    // two in-place transforms, a pointwise pass, the inverse: 88 N): b is transformed OUT OF PLACE into the scratch the reference
    // allocates too (fft/zq.rs:21-25), and the pointwise product rides on the load of the inverse transform.
    StreamWs ws(count * sizeof(u64), st);
    if (ws.rc != FHE_OK) return ws.rc;
    u64 *tb = ws.as<u64>();
    if (n > 1 && mem == FHE_MEM_DEVICE) {
        fhe::NttIo src_b;
        src_b.src = (const u64 *)b; src_b.src_mod = (unsigned)batch;
        rc = fhe::ntt_fwd_multi(ctx->d_desc, 1, tb, log_n, batch, st, ctx->pm_b, src_b);
    } else {  // host operand (or n = 1): the copy is the upload
        hipMemcpyKind kind = mem == FHE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        rc = hipMemcpyAsync(tb, b, count * sizeof(u64), kind, st) == hipSuccess ? FHE_OK : FHE_ERR_HIP;
        if (rc == FHE_OK && n > 1) rc = fhe::ntt_fwd_device(ctx, tb, log_n, batch, st);
    }
    if (rc == FHE_OK && n > 1) {  // forward of a, product, inverse: one launch at 2^13 .. 2^15 (ntt14w_mul_kernel: 40 N bytes in all)
        fhe::NttIo mul_b;
        mul_b.mul = tb; mul_b.mul_div = (unsigned)batch; mul_b.mul_period = (unsigned)batch;
        rc = fhe::ntt_mul_multi(ctx->d_desc, 1, ma.d, log_n, batch, st, ctx->pm_b, mul_b);
    } else if (rc == FHE_OK) {
        rc = launch_pointwise(ctx, ma.d, tb, count, st);  // n = 1: `a[0] *= b[0]`
    }
    if (rc == FHE_OK) rc = ma.sync_out(st);
    return rc;  // tb is released in stream order
}

}  // extern "C"
