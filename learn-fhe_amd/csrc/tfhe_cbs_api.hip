// extern "C" entry points of the circuit bootstrap (k = 1): the private functional key switch TLWE -> TGLWE and the fused
// TLWE bit -> TGGSW rows call.  The key generator fhe_tlwe_pfksk_gen lives in torus_api.hip beside the TGLWE encryption it reuses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>

#include "torus_ctx.hpp"
#include "dispatch.hpp"
#include "pfks_kernels.hpp"
#include "tfhe_cbs.hpp"
#include "tfhe_circuit_kernels.hpp"

namespace {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the product on device buffers; out_a, out_b [batch n_funcs][n] need not be zero
int pfks_dev(const fhe::TDecomp &P, const u64 *key, int n_funcs, const u64 *ct_a, const u64 *ct_b, size_t n_in, size_t n, size_t group, u64 *out_a,
             u64 *out_b, size_t batch, hipStream_t st) {
    const int tile = batch == 1 ? 1 : (batch <= 4 ? 4 : 16);
    const bool bytes = P.log_b <= 7;
    const int vec = (n % 2 == 0 && aligned16(key) && aligned16(out_a) && aligned16(out_b)) ? 2 : 1;
    const size_t rows_in = n_in + 1, W = fhe::pfks_row_words((size_t)n_funcs, n);
    const size_t tiles = (batch + tile - 1) / tile, strips = (W + size_t(fhe::PFKS_THREADS) * vec - 1) / (size_t(fhe::PFKS_THREADS) * vec);
    // a chunk's digit image stays below 48 KiB of LDS; the rule keeps it at PFKS_RULE_CHUNK coefficients (6 KiB at d = 3, TILE = 16, bytes),
    // so that registers, not LDS, set the waves per SIMD; a longer chunk only saves barriers (lab switch PFKS_CHUNK)
    constexpr size_t PFKS_RULE_CHUNK = 128;
    const long lab_chunk = fhe::opt(fhe::OPT_PFKS_CHUNK);
    const size_t chunk_cap = std::max<size_t>(1, std::min<size_t>((48 * 1024) / (size_t(P.d) * tile * (bytes ? 1 : 4)),
                                                                  lab_chunk >= 1 ? (size_t)lab_chunk : PFKS_RULE_CHUNK));
    // the rule: enough blocks for four per compute unit, chunks of at least 32 coefficients; lab switch PFKS_SPLIT: 1 never, k >= 2 k chunks
    size_t z = (size_t(4) * fhe::current_cu_count() + tiles * strips - 1) / (tiles * strips);
    const long forced = fhe::opt(fhe::OPT_PFKS_SPLIT);
    if (forced >= 1) z = (size_t)forced;
    z = std::min<size_t>(std::min<size_t>(z, (rows_in + 31) / 32), 1024);
    z = std::max<size_t>(z, 1);
    size_t chunk = std::min(chunk_cap, (rows_in + z - 1) / z);
    z = std::min(z, (rows_in + chunk - 1) / chunk);  // no block without a chunk
    if (z > 1) {
        HIP_TRY(hipMemsetAsync(out_a, 0, batch * n_funcs * n * sizeof(u64), st));
        HIP_TRY(hipMemsetAsync(out_b, 0, batch * n_funcs * n * sizeof(u64), st));
    }
    const size_t lds = size_t(P.d) * chunk * tile * (bytes ? 1 : 4);
    const fhe::PfksShape S{(unsigned)n_in, (unsigned)n, (unsigned)n_funcs, (unsigned)group, (unsigned)batch, (unsigned)chunk, W};
    const dim3 grid((unsigned)tiles, (unsigned)strips, (unsigned)z);
    return fhe::with_int<1, 4, 16>(tile, [&](auto t) {
        return fhe::with_int<1, 2>(vec, [&](auto v) {
            return fhe::with_bool(bytes, [&](auto b) {
                return fhe::launch<fhe::tlwe_pfks_kernel<decltype(t)::value, decltype(v)::value, decltype(b)::value>>(grid, fhe::PFKS_THREADS, lds, st, ct_a,
                                                                                                                      ct_b, key, S, P, out_a, out_b);
            });
        });
    });
}

}  // namespace

extern "C" {

// include/fhe_ring.h: the private functional key switch
int fhe_tlwe_pfks(int log_b, int d, const uint64_t *pfksk, int n_funcs, const uint64_t *ct_a, const uint64_t *ct_b, size_t n_in, size_t n, size_t group,
                  uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream) {
    int rc = fhe::pfks_check(log_b, d, n_funcs, n_in, n, group, batch);
    if (rc != FHE_OK) return rc;
    if (!pfksk || ((!ct_a || !ct_b || !out_a || !out_b) && batch)) return FHE_ERR_INVALID;
    if (batch && out_a == out_b) return FHE_ERR_INVALID;
    if (batch && mem == FHE_MEM_DEVICE && (out_a == ct_a || out_a == ct_b || out_b == ct_a || out_b == ct_b || out_a == pfksk || out_b == pfksk))
        return FHE_ERR_INVALID;  // the outputs are zeroed or written before every input is read
    if (batch == 0) return FHE_OK;
    PtrDeviceGuard pguard(ct_a, mem);
    if (!pguard.ok) return FHE_ERR_HIP;
    fhe::TDecomp P;
    rc = make_tdecomp(log_b, d, &P);
    if (rc != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t outs = batch * (size_t)n_funcs * n;
    Mirror mk(pfksk, fhe::pfksk_words(d, n_in, (size_t)n_funcs, n), mem, true, st), ma(ct_a, n_in * batch, mem, true, st), mb(ct_b, batch, mem, true, st),
        moa(out_a, outs, mem, false, st), mob(out_b, outs, mem, false, st);
    if (mk.rc | ma.rc | mb.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    rc = pfks_dev(P, mk.d, n_funcs, ma.d, mb.d, n_in, n, group, moa.d, mob.d, batch, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

int fhe_tfhe_cbs_table(int cb_log_b, int cb_d, size_t n, uint64_t *out) { return fhe::cbs_table(cb_log_b, cb_d, n, out); }

int fhe_tfhe_cbs_workspace(size_t n, size_t n_lwe, int cb_d, size_t batch, size_t *words) {
    if (!words || cb_d < 1 || cb_d > fhe::CBS_MAX_D || !fhe::cbs_pow2(n) || n_lwe == 0) return FHE_ERR_INVALID;
    if (n < 256 || n > 2048) return FHE_ERR_UNSUPPORTED;
    *words = fhe::cbs_workspace(n, n_lwe, cb_d, batch);
    return FHE_OK;
}

// include/fhe_ring.h: TLWE bit -> TGGSW rows in one call
int fhe_tfhe_circuit_bootstrap(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int cb_log_b, int cb_d, int pf_log_b, int pf_d, const uint64_t *pfksk,
                               const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t *rows_a, uint64_t *rows_b, size_t batch, fhe_mem mem, void *stream) {
    if (!t || !brk || brk->t != t || !pfksk || ((!lwe_a || !lwe_b || !rows_a || !rows_b) && batch)) return FHE_ERR_INVALID;
    const size_t n = size_t(1) << brk->log_n, n_lwe = brk->count;
    int rc = fhe::cbs_check(cb_log_b, cb_d, n);
    if (rc != FHE_OK) return rc;
    if (batch > 0x7fffffffull / (2 * (size_t)cb_d)) return FHE_ERR_UNSUPPORTED;
    rc = fhe::pfks_check(pf_log_b, pf_d, 2, n, n, (size_t)cb_d, batch * cb_d);
    if (rc != FHE_OK) return rc;
    if (batch && rows_a == rows_b) return FHE_ERR_INVALID;
    if (batch && mem == FHE_MEM_DEVICE)  // the rows must not overlap an input or the key
        for (const uint64_t *o : {(const uint64_t *)rows_a, (const uint64_t *)rows_b})
            if (o == lwe_a || o == lwe_b || o == pfksk) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    fhe::TDecomp P;
    rc = make_tdecomp(pf_log_b, pf_d, &P);
    if (rc != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const int nu = fhe::cbs_nu(cb_d);
    const size_t levels = batch * cb_d, outs = 2 * levels * n;
    Mirror mk(pfksk, fhe::pfksk_words(pf_d, n, 2, n), mem, true, st), ma(lwe_a, n_lwe * batch, mem, true, st), mb(lwe_b, batch, mem, true, st),
        moa(rows_a, outs, mem, false, st), mob(rows_b, outs, mem, false, st);
    if (mk.rc | ma.rc | mb.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    const fhe::TfheScratch L = fhe::cbs_scratch(n, n_lwe, cb_d, batch);  // then the table [n]
    StreamWs wsp((L.total + n) * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ws = wsp.as<u64>(), *ra = ws + L.acc_a, *rb = ws + L.acc_b, *ea = ws + L.ext_a, *eb = ws + L.ext_b, *at = ws + L.at, *bt = ws + L.bt;
    u64 *tab = ws + L.total;
    typedef uint64_t U;
    rc = fhe::launch<fhe::cbs_table_kernel>(grid_for(n), 256, 0, st, tab, (unsigned)n, nu, cb_log_b, cb_d);
    if (rc == FHE_OK) rc = fhe_tfhe_mod_switch_many((const U *)ma.d, (U *)at, batch * n_lwe, n, nu, FHE_MEM_DEVICE, stream);
    if (rc == FHE_OK) rc = fhe_tfhe_mod_switch_many((const U *)mb.d, (U *)bt, batch, n, nu, FHE_MEM_DEVICE, stream);
    if (rc == FHE_OK) rc = fhe_tfhe_blind_rotate(t, brk, (const U *)at, (const U *)bt, (const U *)tab, (U *)ra, (U *)rb, batch, FHE_MEM_DEVICE, stream);
    // tglwe.rs:115-127 for the indices 0 .. cb_d - 1 alone: [batch][cb_d][n], the key switch's input order
    if (rc == FHE_OK) rc = fhe::launch_sample_extract_many(ra, rb, n, 1, batch, nullptr, nullptr, 0, (size_t)cb_d, 1, (size_t)cb_d, ea, eb, st);
    if (rc == FHE_OK) rc = pfks_dev(P, mk.d, 2, ea, eb, n, n, (size_t)cb_d, moa.d, mob.d, levels, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

}  // extern "C"
