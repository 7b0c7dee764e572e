// extern "C" entry points of the CKKS encoder: scheme/ckks/src/ckks.rs:186-213 `Ckks::encode` / `Ckks::decode` and the transforms under
// them, scheme/ckks/src/sfft.rs:7-72 `sfft` / `sifft` / `w`, in double-double arithmetic (dd.hpp) in place of the reference's 256-bit
// software floats.  Routes (ckks_encode_kernels.hpp): l = n / 2 <= 4096 runs one LDS kernel, one message per workgroup; l = 8192 and
// 16384 run the top one or two stages in registers and the rest in LDS chunks of 4096, through a stream-ordered workspace of 32 l
// bytes per message.  Encode and decode fuse their integer ends into the same kernels.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "api_common.hpp"
#include "ckks_encode_kernels.hpp"
#include "ckks_encoder.hpp"
#include "dispatch.hpp"
#include "modmath.hpp"
#include "rns_ctx.hpp"

namespace {
using fhe::EncTables;

unsigned lds_grid(size_t chunks) { return (unsigned)(chunks > (size_t(1) << 20) ? (size_t(1) << 20) : chunks); }

// one pass of sfft_lds_kernel over `msgs` messages cut into chunks of 2^log_c
template <bool INV, class Src, class Dst>
int run_lds(const fhe_ckks_encoder *e, Src src, Dst dst, int log_c, size_t msgs, hipStream_t st) {
    const EncTables T{e->d_tw, e->d_pow5, (unsigned)e->log_l};
    const size_t chunks = msgs << (e->log_l - log_c);
    const unsigned threads = log_c >= 10 ? 512 : 256;
    return fhe::launch<fhe::sfft_lds_kernel<INV, Src, Dst>>(lds_grid(chunks), threads, (size_t(32) << log_c), st, src, dst, T, (unsigned)log_c, chunks);
}
template <bool INV, class Src, class Dst>
int run_top(const fhe_ckks_encoder *e, Src src, Dst dst, size_t msgs, hipStream_t st) {
    const EncTables T{e->d_tw, e->d_pow5, (unsigned)e->log_l};
    const int s = e->log_l - fhe::ENC_LDS_LOG_C;
    return fhe::with_int<1, 2>(s, [&](auto S) {
        return fhe::launch<fhe::sfft_top_kernel<INV, S(), Src, Dst>>(grid_for((msgs << e->log_l) >> S()), 256, 0, st, src, dst, T, msgs);
    });
}
// sifft from `src` into `dst`
template <class Src, class Dst>
int run_sifft(const fhe_ckks_encoder *e, Src src, Dst dst, size_t msgs, hipStream_t st) {
    if (e->log_l <= fhe::ENC_LDS_LOG_C) return run_lds<true>(e, src, dst, e->log_l, msgs, st);
    StreamWs ws((msgs << e->log_l) * sizeof(double4), st);
    if (ws.rc != FHE_OK) return ws.rc;
    FHE_TRY(run_top<true>(e, src, fhe::WsOut{ws.as<double4>(), e->l}, msgs, st));
    return run_lds<true>(e, fhe::WsIn{ws.as<double4>(), e->l}, dst, fhe::ENC_LDS_LOG_C, msgs, st);
}
template <class Src, class Dst>
int run_sfft(const fhe_ckks_encoder *e, Src src, Dst dst, size_t msgs, hipStream_t st) {
    if (e->log_l <= fhe::ENC_LDS_LOG_C) return run_lds<false>(e, src, dst, e->log_l, msgs, st);
    StreamWs ws((msgs << e->log_l) * sizeof(double4), st);
    if (ws.rc != FHE_OK) return ws.rc;
    FHE_TRY(run_lds<false>(e, src, fhe::WsOut{ws.as<double4>(), e->l}, fhe::ENC_LDS_LOG_C, msgs, st));
    return run_top<false>(e, fhe::WsIn{ws.as<double4>(), e->l}, dst, msgs, st);
}

// handle checks shared by the compute entries; a host-only encoder computes nothing
int compute_ok(const fhe_ckks_encoder *e) { return (e && e->device >= 0) ? FHE_OK : FHE_ERR_INVALID; }
int pair_ok(const fhe_ckks_encoder *e, const fhe_rns_ctx *r, uint64_t scale) {
    if (compute_ok(e) != FHE_OK || !r || r->device != e->device || scale == 0) return FHE_ERR_INVALID;
    return FHE_OK;
}
// The largest array of a call is batch * limbs * n words of 8 bytes (limbs = 4 for the slot arrays' 32 bytes per element would be
// smaller than any L >= 2, so callers pass max(L, 4)): its byte count batch * limbs * 2^(log_l + 4) must stay below 2^62, that is
// batch * limbs < 2^(58 - log_l).  All kernel offsets are size_t; this only keeps the host's size arithmetic from wrapping.
bool too_many(const fhe_ckks_encoder *e, size_t batch, size_t limbs) { return batch > (size_t(1) << (58 - e->log_l)) / limbs; }

int transform(const fhe_ckks_encoder *e, double *z_hi, double *z_lo, size_t batch, fhe_mem mem, void *stream, bool inverse) {
    if (compute_ok(e) != FHE_OK) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!z_hi) return FHE_ERR_INVALID;
    if (too_many(e, batch, 4)) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(e->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = batch * e->l * 2;
    Mirror mh(z_hi, words, mem, true, st), ml(z_lo, z_lo ? words : 0, mem, true, st);
    if (mh.rc | ml.rc) return FHE_ERR_HIP;
    const fhe::ZIn src{(const double2 *)mh.d, (const double2 *)ml.d, e->l};
    const fhe::ZOut dst{(double2 *)mh.d, (double2 *)ml.d, e->l};
    FHE_TRY(inverse ? run_sifft(e, src, dst, batch, st) : run_sfft(e, src, dst, batch, st));
    int rc = mh.sync_out(st);
    return rc != FHE_OK ? rc : ml.sync_out(st);
}
}  // namespace

int fhe::ckks_encode_diag_rot(const fhe_ckks_encoder *e, const fhe_rns_ctx *rns, uint64_t scale, fhe::DiagRotIn src, size_t msgs, u64 *pt, hipStream_t st) {
    if (pair_ok(e, rns, scale) != FHE_OK || !pt) return FHE_ERR_INVALID;
    if (msgs == 0) return FHE_OK;
    if (too_many(e, msgs, rns->L < 4 ? 4 : (size_t)rns->L)) return FHE_ERR_UNSUPPORTED;
    const fhe::EncodeTail dst{pt, e->l, (unsigned)rns->L, rns->d_barrett, rns->resc.red_mu, fhe::ddm::from_u64(scale), e->d_status};
    return run_sifft(e, src, dst, msgs, st);
}

extern "C" {

void fhe_ckks_encoder_destroy(fhe_ckks_encoder *e) {
    if (!e) return;
    if (e->device >= 0) {
        DeviceGuard guard(e->device);
        if (e->d_tw) (void)hipFree(e->d_tw);
        if (e->d_pow5) (void)hipFree(e->d_pow5);
        if (e->d_status) (void)hipFree(e->d_status);
    }
    delete e;
}

int fhe_ckks_encoder_create(size_t n, int device, fhe_ckks_encoder **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!is_pow2(n) || n < 2 || n > (size_t(2) << fhe::ENC_MAX_LOG_L)) return FHE_ERR_INVALID;
    fhe_ckks_encoder *e = new (std::nothrow) fhe_ckks_encoder();
    if (!e) return FHE_ERR_INVALID;
    e->n = n; e->l = (unsigned)(n / 2); e->log_l = ilog2(n / 2); e->device = device < 0 ? -1 : device;
    try {  // the tables are std::vectors: no exception crosses the C boundary (out of memory is FHE_ERR_INVALID here as for the handle)
        e->tw.resize(4 * size_t(e->l));
        fhe::ddm::twiddle_table(e->l, e->tw.data());
        e->pow5.resize(e->l / 2 ? e->l / 2 : 1);
        fhe::ddm::pow5_table(e->l, e->pow5.data());
    } catch (const std::bad_alloc &) {
        delete e;
        return FHE_ERR_INVALID;
    }
    if (device >= 0) {
        static_assert(sizeof(fhe::cdd) == sizeof(double4), "a table entry is (re.hi, re.lo, im.hi, im.lo)");
        DeviceGuard guard(device);
        int rc = guard.ok ? FHE_OK : FHE_ERR_HIP;
        hipError_t err = hipSuccess;
        if (rc == FHE_OK) err = hipMalloc((void **)&e->d_tw, e->tw.size() * sizeof(double4));
        if (rc == FHE_OK && err == hipSuccess) err = hipMalloc((void **)&e->d_pow5, e->pow5.size() * sizeof(unsigned));
        if (rc == FHE_OK && err == hipSuccess) err = hipMalloc((void **)&e->d_status, sizeof(int));
        if (rc == FHE_OK && err == hipSuccess) err = hipMemcpy(e->d_tw, e->tw.data(), e->tw.size() * sizeof(double4), hipMemcpyHostToDevice);
        if (rc == FHE_OK && err == hipSuccess) err = hipMemcpy(e->d_pow5, e->pow5.data(), e->pow5.size() * sizeof(unsigned), hipMemcpyHostToDevice);
        if (rc == FHE_OK && err == hipSuccess) err = hipMemset(e->d_status, 0, sizeof(int));
        if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; }
        if (rc != FHE_OK) { fhe_ckks_encoder_destroy(e); return rc; }
    }
    *out = e;
    return FHE_OK;
}

int fhe_ckks_encoder_twiddles(const fhe_ckks_encoder *e, double *out, size_t count) {
    if (!e || (!out && count) || count > e->tw.size()) return FHE_ERR_INVALID;
    for (size_t i = 0; i < count; ++i) {
        const fhe::cdd t = e->tw[i];
        out[4 * i] = t.re.hi; out[4 * i + 1] = t.re.lo; out[4 * i + 2] = t.im.hi; out[4 * i + 3] = t.im.lo;
    }
    return FHE_OK;
}

int fhe_ckks_encoder_status(const fhe_ckks_encoder *e, void *stream, int clear) {
    if (compute_ok(e) != FHE_OK) return FHE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(e->device);
    if (!guard.ok) return FHE_ERR_HIP;
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, e->d_status, sizeof(int), hipMemcpyDeviceToHost, st));
    if (clear) HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), st));
    HIP_TRY(hipStreamSynchronize(st));
    return h ? FHE_ERR_INVALID : FHE_OK;
}

int fhe_ckks_sifft(const fhe_ckks_encoder *e, double *z_hi, double *z_lo, size_t batch, fhe_mem mem, void *stream) {
    return transform(e, z_hi, z_lo, batch, mem, stream, true);
}
int fhe_ckks_sfft(const fhe_ckks_encoder *e, double *z_hi, double *z_lo, size_t batch, fhe_mem mem, void *stream) {
    return transform(e, z_hi, z_lo, batch, mem, stream, false);
}

int fhe_ckks_encode(const fhe_ckks_encoder *e, const fhe_rns_ctx *rns, uint64_t scale, const double *m_hi, const double *m_lo, size_t batch,
                    uint64_t *pt, fhe_mem mem, void *stream) {
    if (pair_ok(e, rns, scale) != FHE_OK) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!m_hi || !pt) return FHE_ERR_INVALID;
    const size_t L = rns->L;
    if (too_many(e, batch, L < 4 ? 4 : L)) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(e->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = batch * e->l * 2;
    Mirror mh(m_hi, words, mem, true, st), ml(m_lo, m_lo ? words : 0, mem, true, st), mp(pt, batch * L * e->n, mem, false, st);
    if (mh.rc | ml.rc | mp.rc) return FHE_ERR_HIP;
    const fhe::ZIn src{(const double2 *)mh.d, (const double2 *)ml.d, e->l};
    const fhe::EncodeTail dst{mp.d, e->l, (unsigned)L, rns->d_barrett, rns->resc.red_mu, fhe::ddm::from_u64(scale), e->d_status};
    FHE_TRY(run_sifft(e, src, dst, batch, st));
    int rc = mp.sync_out(st);
    // a host-memory call has synchronised: it reports an out-of-range slot in its return value (and clears the word)
    if (rc == FHE_OK && mem == FHE_MEM_HOST) rc = fhe_ckks_encoder_status(e, stream, 1);
    return rc;
}

int fhe_ckks_decode(const fhe_ckks_encoder *e, const fhe_rns_ctx *rns, uint64_t scale, const uint64_t *pt, size_t batch, double *m_hi, double *m_lo,
                    fhe_mem mem, void *stream) {
    if (pair_ok(e, rns, scale) != FHE_OK) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!m_hi || !pt) return FHE_ERR_INVALID;
    const int L = rns->L;
    if (too_many(e, batch, L < 4 ? 4 : (size_t)L)) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(e->device);
    if (!guard.ok) return FHE_ERR_HIP;
    // Garner's constants and Q of this context (L^2 host multiplications per call)
    fhe::DecodeConsts K{};
    K.big_q[0] = 1;
    for (int i = 0; i < L; ++i) {
        const uint64_t q = rns->qs[i];
        K.q[i] = q;
        uint64_t prod = 1 % q;
        for (int j = 0; j < i; ++j) prod = fhe::mulmod(prod, rns->qs[j] % q, q);
        if (i && prod == 0) return FHE_ERR_INVALID;  // a repeated modulus: no mixed-radix form
        K.cinv[i] = i ? fhe::invmod(prod, q) : 1;
        uint64_t carry = 0;
        for (int k = 0; k < L; ++k) {
            const fhe::u128 t = (fhe::u128)K.big_q[k] * q + carry;
            K.big_q[k] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
    }
    const size_t words = batch * e->l * 2;
    Mirror mp(pt, batch * size_t(L) * e->n, mem, true, st), mh(m_hi, words, mem, false, st), ml(m_lo, m_lo ? words : 0, mem, false, st);
    if (mh.rc | ml.rc | mp.rc) return FHE_ERR_HIP;
    const fhe::ZOut dst{(double2 *)mh.d, (double2 *)ml.d, e->l};
    FHE_TRY(fhe::with_limb_bound(L, [&](auto M, auto) {
        const fhe::DecodeHead<M()> src{mp.d, e->l, (unsigned)L, rns->d_barrett, rns->resc.red_mu, fhe::ddm::from_u64(scale), e->d_status, K};
        return run_sfft(e, src, dst, batch, st);
    }));
    int rc = mh.sync_out(st);
    if (rc == FHE_OK) rc = ml.sync_out(st);
    if (rc == FHE_OK && mem == FHE_MEM_HOST) rc = fhe_ckks_encoder_status(e, stream, 1);
    return rc;
}

}  // extern "C"
