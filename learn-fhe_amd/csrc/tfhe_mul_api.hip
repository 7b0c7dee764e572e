// extern "C" entry points of the TGLWE ciphertext product (k = 1): the relinearisation key (generation, prepared form) and the tensor,
// the relinearisation and the two fused.  include/fhe_ring.h has the definitions; tfhe_mul.hpp the rules that need no device.
#include <hip/hip_runtime.h>

#include <new>

#include "torus_ctx.hpp"
#include "dispatch.hpp"
#include "torus_dispatch.hpp"
#include "tfhe_mul.hpp"
#include "tfhe_mul_kernels.hpp"
#include "tglwe_key_rows.hpp"

// The rows of a relinearisation key in the evaluation domain of the two 60-bit primes: per prime [d][2][n], key_perm layout.
struct fhe_tglwe_relin_key {
    const fhe_torus_ctx *t = nullptr;
    int device = -1;  // t's device, kept here: destroying the key must not read a context that may be gone already
    int log_n = 0;
    u64 *d_rows[2] = {nullptr, nullptr};  // one allocation
    fhe::TDecomp P{};
};

namespace {

inline bool batch_fits(size_t batch) { return batch <= 0x7fffffffull; }

// [a, a + words) and [b, b + words) share a word
inline bool ranges_overlap(const uint64_t *a, const uint64_t *b, size_t words) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)words * sizeof(uint64_t);
    return x < y ? y - x < len : x - y < len;
}

fhe::RelinKeyArg key_arg(const fhe_tglwe_relin_key *key) { return fhe::RelinKeyArg{key->d_rows[0], key->d_rows[1], key->t->T, key->P}; }

template <class W>
unsigned team_blocks(size_t batch) { return (unsigned)((batch + W::TEAMS - 1) / W::TEAMS); }

int tensor_dev(const fhe_torus_ctx *t, int log_n, const u64 *a1, const u64 *b1, const u64 *a2, const u64 *b2, int log_delta, u64 *c0, u64 *c1, u64 *c2,
               size_t batch, hipStream_t st) {
    return with_torus<TorusRing>(log_n, [&](auto wr) {
        using W = typename decltype(wr)::type;
        return fhe::launch<fhe::tglwe_tensor_kernel<W>>(team_blocks<W>(batch), W::THREADS, fhe::mul_lds_bytes<W>(), st, a1, b1, a2, b2, log_delta, t->T, c0,
                                                        c1, c2, (unsigned)batch);
    });
}

int relin_dev(const fhe_tglwe_relin_key *key, const u64 *c0, const u64 *c1, const u64 *c2, u64 *out_a, u64 *out_b, size_t batch, hipStream_t st) {
    return with_torus<TorusRing>(key->log_n, [&](auto wr) {
        using W = typename decltype(wr)::type;
        return fhe::launch<fhe::tglwe_relin_kernel<W>>(team_blocks<W>(batch), W::THREADS, W::TORUS_LDS_BYTES, st, key_arg(key), c0, c1, c2, out_a, out_b,
                                                       (unsigned)batch);
    });
}

int mul_dev(const fhe_tglwe_relin_key *key, const u64 *a1, const u64 *b1, const u64 *a2, const u64 *b2, int log_delta, u64 *out_a, u64 *out_b,
            size_t batch, hipStream_t st) {
    return with_torus<TorusRing>(key->log_n, [&](auto wr) {
        using W = typename decltype(wr)::type;
        return fhe::launch<fhe::tglwe_mul_kernel<W>>(team_blocks<W>(batch), W::THREADS, fhe::mul_lds_bytes<W>(), st, key_arg(key), a1, b1, a2, b2, log_delta,
                                                     out_a, out_b, (unsigned)batch);
    });
}

}  // namespace

extern "C" {

// include/fhe_ring.h: S^2 and the rows h_j S^2 on the device, then fhe_tglwe_sk_encrypt on them
int fhe_tglwe_rlk_gen(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *sk, size_t n, double std_dev, const fhe_rng *rng, uint64_t stream_id,
                      uint64_t *rlk_a, uint64_t *rlk_b, fhe_mem mem, void *stream) {
    if (!t || !sk || !rng || !rlk_a || !rlk_b || !(std_dev >= 0)) return FHE_ERR_INVALID;
    const int rc0 = fhe::mul_gadget_check(log_b, d, n);
    if (rc0 != FHE_OK) return rc0;
    if (t->device < 0) return FHE_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = size_t(d) * n;
    Mirror msk(sk, n, mem, true, st), ma(rlk_a, words, mem, false, st), mb(rlk_b, words, mem, false, st);
    if (msk.rc | ma.rc | mb.rc) return FHE_ERR_HIP;
    StreamWs wsp(words * sizeof(u64), st);  // the plaintext rows
    if (wsp.rc != FHE_OK) return wsp.rc;
    FHE_TRY(fhe::launch<fhe::rlk_plain_kernel>(grid_for(n), 256, 0, st, (const u64 *)msk.d, (unsigned)n, log_b, d, wsp.as<u64>()));
    int rc = fhe_tglwe_sk_encrypt(t, (const uint64_t *)msk.d, (const uint64_t *)wsp.as<u64>(), n, (size_t)d, std_dev, rng, stream_id, (uint64_t *)ma.d,
                                  (uint64_t *)mb.d, FHE_MEM_DEVICE, stream);
    if (rc == FHE_OK) rc = ma.sync_out(st);
    if (rc == FHE_OK) rc = mb.sync_out(st);
    return rc;
}

void fhe_tglwe_rlk_destroy(fhe_tglwe_relin_key *key) {
    if (!key) return;
    if (key->device >= 0 && key->d_rows[0]) {
        DeviceGuard guard(key->device);
        (void)hipFree(key->d_rows[0]);
    }
    delete key;
}

// include/fhe_ring.h: the d rows, once, into the evaluation domain of the two 60-bit primes
int fhe_tglwe_rlk_prepare(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *rlk_a, const uint64_t *rlk_b, size_t n, fhe_mem mem, void *stream,
                          fhe_tglwe_relin_key **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!t || !rlk_a || !rlk_b) return FHE_ERR_INVALID;
    int rc = fhe::mul_gadget_check(log_b, d, n);
    if (rc != FHE_OK) return rc;
    fhe::TDecomp P;
    rc = make_tdecomp(log_b, d, &P);
    if (rc != FHE_OK) return rc;
    if (t->device < 0) return FHE_ERR_NO_DEVICE;
    const int log_n = ilog2(n);
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t half = size_t(d) * n, words = 2 * half;  // of one prime
    fhe_tglwe_relin_key *k = new (std::nothrow) fhe_tglwe_relin_key();
    if (!k) return FHE_ERR_INVALID;
    k->t = t; k->device = t->device; k->log_n = log_n; k->P = P;
    if (hipMalloc((void **)&k->d_rows[0], 2 * words * sizeof(u64)) != hipSuccess) { (void)hipGetLastError(); delete k; return FHE_ERR_HIP; }
    k->d_rows[1] = k->d_rows[0] + words;
    {
        Mirror ma(rlk_a, half, mem, true, st), mb(rlk_b, half, mem, true, st);
        rc = (ma.rc | mb.rc) ? FHE_ERR_HIP : tglwe_rows_prepare(t, log_n, ma.d, mb.d, (size_t)d, k->d_rows, st);
        // the key may serve calls on any stream from here on: wait for its rows (and, with them, for the staging copies)
        if (hipStreamSynchronize(st) != hipSuccess && rc == FHE_OK) { (void)hipGetLastError(); rc = FHE_ERR_HIP; }
    }
    if (rc != FHE_OK) { fhe_tglwe_rlk_destroy(k); return rc; }
    *out = k;
    return FHE_OK;
}

// include/fhe_ring.h: the three polynomials of the tensor
int fhe_tglwe_tensor(const fhe_torus_ctx *t, const uint64_t *ct0_a, const uint64_t *ct0_b, const uint64_t *ct1_a, const uint64_t *ct1_b, size_t n,
                     int log_delta, uint64_t *c0, uint64_t *c1, uint64_t *c2, size_t batch, fhe_mem mem, void *stream) {
    if (!t || !ct0_a || !ct0_b || !ct1_a || !ct1_b || !c0 || !c1 || !c2) return FHE_ERR_INVALID;
    if (n != 256 && n != 512 && n != 1024 && n != 2048) return FHE_ERR_INVALID;
    if (fhe::mul_log_delta_check(log_delta) != FHE_OK) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!batch_fits(batch)) return FHE_ERR_UNSUPPORTED;
    {  // no output may overlap an input or another output, in any word of the batch n words each covers
        const uint64_t *outs[3] = {c0, c1, c2}, *all[7] = {c0, c1, c2, ct0_a, ct0_b, ct1_a, ct1_b};
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 7; ++j)
                if (ranges_overlap(outs[i], all[j], batch * n)) return FHE_ERR_INVALID;
    }
    if (t->device < 0) return FHE_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = batch * n;
    Mirror m0a(ct0_a, words, mem, true, st), m0b(ct0_b, words, mem, true, st), m1a(ct1_a, words, mem, true, st), m1b(ct1_b, words, mem, true, st),
        mc0(c0, words, mem, false, st), mc1(c1, words, mem, false, st), mc2(c2, words, mem, false, st);
    if (m0a.rc | m0b.rc | m1a.rc | m1b.rc | mc0.rc | mc1.rc | mc2.rc) return FHE_ERR_HIP;
    int rc = tensor_dev(t, ilog2(n), m0a.d, m0b.d, m1a.d, m1b.d, log_delta, mc0.d, mc1.d, mc2.d, batch, st);
    if (rc == FHE_OK) rc = mc0.sync_out(st);
    if (rc == FHE_OK) rc = mc1.sync_out(st);
    if (rc == FHE_OK) rc = mc2.sync_out(st);
    return rc;
}

// include/fhe_ring.h: (c0, c1, c2) -> a two-polynomial ciphertext
int fhe_tglwe_relin(const fhe_torus_ctx *t, const fhe_tglwe_relin_key *key, const uint64_t *c0, const uint64_t *c1, const uint64_t *c2, uint64_t *out_a,
                    uint64_t *out_b, size_t batch, fhe_mem mem, void *stream) {
    if (!t || !key || key->t != t || !c0 || !c1 || !c2 || !out_a || !out_b || out_a == out_b) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!batch_fits(batch)) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = batch << key->log_n;
    Mirror m0(c0, words, mem, true, st), m1(c1, words, mem, true, st), m2(c2, words, mem, true, st), moa(out_a, words, mem, false, st),
        mob(out_b, words, mem, false, st);
    if (m0.rc | m1.rc | m2.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    int rc = relin_dev(key, m0.d, m1.d, m2.d, moa.d, mob.d, batch, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

// include/fhe_ring.h: relin(tensor(ct0, ct1, log_delta)), one launch
int fhe_tglwe_mul(const fhe_torus_ctx *t, const fhe_tglwe_relin_key *key, const uint64_t *ct0_a, const uint64_t *ct0_b, const uint64_t *ct1_a,
                  const uint64_t *ct1_b, int log_delta, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream) {
    if (!t || !key || !ct0_a || !ct0_b || !ct1_a || !ct1_b || !out_a || !out_b || out_a == out_b) return FHE_ERR_INVALID;
    if (fhe::mul_log_delta_check(log_delta) != FHE_OK || key->t != t) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!batch_fits(batch)) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = batch << key->log_n;
    Mirror m0a(ct0_a, words, mem, true, st), m0b(ct0_b, words, mem, true, st), m1a(ct1_a, words, mem, true, st), m1b(ct1_b, words, mem, true, st),
        moa(out_a, words, mem, false, st), mob(out_b, words, mem, false, st);
    if (m0a.rc | m0b.rc | m1a.rc | m1b.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    int rc = mul_dev(key, m0a.d, m0b.d, m1a.d, m1b.d, log_delta, moa.d, mob.d, batch, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

}  // extern "C"
