// extern "C" entry points of the packing key switch (k = 1): the prepared form of a one-function private functional key-switch key and
// the call that packs TLWE ciphertexts into TGLWE ciphertexts.  The key itself comes from fhe_tlwe_pfksk_gen (torus_api.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "torus_ctx.hpp"
#include "dispatch.hpp"
#include "torus_dispatch.hpp"
#include "tfhe_pack.hpp"
#include "tfhe_pack_kernels.hpp"

// The rows of a packing key, as they came and in the evaluation domain of the two 60-bit primes: per prime [d (n_in + 1)][2][n], key_perm layout.
struct fhe_tlwe_pack_key {
    const fhe_torus_ctx *t = nullptr;
    int device = -1;  // t's device, kept here: destroying the key must not read a context that may be gone already
    int log_n = 0;
    size_t n_in = 0, rows = 0;
    u64 *d_raw = nullptr;                 // the rows as they came, [rows][1][2][n]: the key of the scalar route (fhe_tlwe_pfks)
    u64 *d_rows[2] = {nullptr, nullptr};  // the two primes' planes, behind d_raw in its allocation
    fhe::TDecomp P{};
};

namespace {

constexpr size_t PACK_SLAB_BYTES = size_t(256) << 20;  // scratch of the packs one launch group works on (digit polynomials, or the scalar route's rows)

// f(Type<digit type>{}) for the width pack_digit_bytes gives
template <class F>
int with_digit(int log_b, F &&f) {
    const int w = fhe::pack_digit_bytes(log_b);
    if (w == 1) return f(fhe::Type<signed char>{});
    if (w == 2) return f(fhe::Type<short>{});
    return f(fhe::Type<int>{});
}

// The scalar route on device buffers: fhe_tlwe_pfks under the raw rows (one function, group 1) on the inputs of a group of packs, then
// one kernel that rotates result r of every pack by r stride and sums
int pack_scalar_dev(const fhe_tlwe_pack_key *key, const u64 *ct_a, const u64 *ct_b, size_t count, size_t stride, size_t packs, u64 *out_a, u64 *out_b,
                    hipStream_t st) {
    const size_t n = size_t(1) << key->log_n, per_pack = 2 * count * n * sizeof(u64);
    const size_t slab = fhe::pack_slab(packs, per_pack, PACK_SLAB_BYTES, 0x7fffffffull / count, fhe::opt(fhe::OPT_PACK_SLAB));
    StreamWs wsp(slab * per_pack, st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    for (size_t g0 = 0; g0 < packs; g0 += slab) {
        const size_t gs = std::min(slab, packs - g0);
        u64 *ta = wsp.as<u64>(), *tb = ta + gs * count * n;
        FHE_TRY(fhe_tlwe_pfks(key->P.log_b, key->P.d, (const uint64_t *)key->d_raw, 1, (const uint64_t *)(ct_a + g0 * count * key->n_in), (const uint64_t *)(ct_b + g0 * count),
                              key->n_in, n, 1, (uint64_t *)ta, (uint64_t *)tb, gs * count,
                              FHE_MEM_DEVICE, (void *)st));
        FHE_TRY(fhe::launch<fhe::tlwe_pack_gather_kernel>(grid_for(2 * gs * n), 256, 0, st, (const u64 *)ta, (const u64 *)tb, (unsigned)n, (unsigned)count,
                                                          (unsigned)stride, gs, out_a + g0 * n, out_b + g0 * n));
    }
    return FHE_OK;
}

// packs on device buffers: out_a, out_b [packs][n] need not be zero
int pack_dev(const fhe_tlwe_pack_key *key, const u64 *ct_a, const u64 *ct_b, size_t count, size_t stride, size_t packs, u64 *out_a, u64 *out_b,
             hipStream_t st) {
    if (count == 1) stride = 1;  // the one input lands at coefficient 0
    if (fhe::pack_scalar_route(count, fhe::opt(fhe::OPT_PACK_ROUTE))) return pack_scalar_dev(key, ct_a, ct_b, count, stride, packs, out_a, out_b, st);
    const size_t n = size_t(1) << key->log_n, rows = key->rows;
    const fhe::PackPlan plan = fhe::pack_plan(rows, key->log_n, key->P.log_b, packs, (size_t)fhe::current_cu_count(), fhe::opt(fhe::OPT_PACK_SPLIT));
    if (plan.chunks == 0) return FHE_ERR_UNSUPPORTED;
    const size_t dw = (size_t)fhe::pack_digit_bytes(key->P.log_b), per_pack = rows * n * dw;
    const size_t slab = fhe::pack_slab(packs, per_pack, PACK_SLAB_BYTES, 65535, fhe::opt(fhe::OPT_PACK_SLAB));  // 65535: grid z of the front pass
    StreamWs wsp(slab * per_pack, st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    if (plan.chunks > 1) {
        HIP_TRY(hipMemsetAsync(out_a, 0, packs * n * sizeof(u64), st));
        HIP_TRY(hipMemsetAsync(out_b, 0, packs * n * sizeof(u64), st));
    }
    const bool dense = stride == 1 && count == n;  // every coefficient of every digit polynomial is written
    const fhe::PackKeyArg karg{key->d_rows[0], key->d_rows[1], key->t->T};
    for (size_t g0 = 0; g0 < packs; g0 += slab) {
        const size_t gs = std::min(slab, packs - g0);
        if (!dense) HIP_TRY(hipMemsetAsync(wsp.p, 0, gs * per_pack, st));
        const fhe::PackShape S{(unsigned)key->n_in, (unsigned)n, (unsigned)count, (unsigned)stride, (unsigned)rows};
        const dim3 fgrid((unsigned)((key->n_in + 1 + fhe::PACK_TILE - 1) / fhe::PACK_TILE), (unsigned)((count + fhe::PACK_TILE - 1) / fhe::PACK_TILE),
                         (unsigned)gs);
        const u64 *ca = ct_a + g0 * count * key->n_in, *cb = ct_b + g0 * count;
        u64 *oa = out_a + g0 * n, *ob = out_b + g0 * n;
        if (gs * (plan.chunks + fhe::PACK_DIES) > 0x7fffffffull) return FHE_ERR_UNSUPPORTED;
        const int rc = with_digit(key->P.log_b, [&](auto dt) {
            using D = typename decltype(dt)::type;
            D *dig = wsp.as<D>();
            FHE_TRY(fhe::launch<fhe::tlwe_pack_digits_kernel<D>>(fgrid, 256, 0, st, ca, cb, dig, S, key->P));
            return with_torus<TorusRing>(key->log_n, [&](auto wr) {
                using W = typename decltype(wr)::type;
                return fhe::launch<fhe::tlwe_pack_kernel<W, D>>((unsigned)fhe::pack_team_blocks<W>(plan.chunks, gs), W::THREADS, W::TORUS_LDS_BYTES, st,
                                                                (const D *)dig, karg, (unsigned)rows, (unsigned)plan.per_chunk, (unsigned)plan.chunks,
                                                                (unsigned)gs, oa, ob);
            });
        });
        if (rc != FHE_OK) return rc;
    }
    return FHE_OK;
}

}  // namespace

extern "C" {

void fhe_tlwe_pack_key_destroy(fhe_tlwe_pack_key *key) {
    if (!key) return;
    if (key->device >= 0 && key->d_raw) {
        DeviceGuard guard(key->device);
        (void)hipFree(key->d_raw);
    }
    delete key;
}

// include/fhe_ring.h: the rows of a one-function key, once, into the evaluation domain of the two 60-bit primes; a copy of the rows as they
// came stays with them for the scalar route
int fhe_tlwe_pack_key_prepare(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *pfksk, size_t n_in, size_t n, fhe_mem mem, void *stream,
                              fhe_tlwe_pack_key **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!t || !pfksk) return FHE_ERR_INVALID;
    int rc = fhe::pack_key_check(log_b, d, n_in, n);
    if (rc != FHE_OK) return rc;
    fhe::TDecomp P;
    rc = make_tdecomp(log_b, d, &P);
    if (rc != FHE_OK) return rc;
    const int log_n = ilog2(n);
    if (fhe::pack_max_rows(log_n, log_b) == 0) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t rows = size_t(d) * (n_in + 1), polys = 2 * rows, words = polys * n;  // of the raw rows, and of one prime
    fhe_tlwe_pack_key *k = new (std::nothrow) fhe_tlwe_pack_key();
    if (!k) return FHE_ERR_INVALID;
    k->t = t; k->device = t->device; k->log_n = log_n; k->n_in = n_in; k->rows = rows; k->P = P;
    if (hipMalloc((void **)&k->d_raw, 3 * words * sizeof(u64)) != hipSuccess) { (void)hipGetLastError(); delete k; return FHE_ERR_HIP; }
    k->d_rows[0] = k->d_raw + words;
    k->d_rows[1] = k->d_raw + 2 * words;
    if (hipMemcpyAsync(k->d_raw, pfksk, words * sizeof(u64), mem == FHE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st) != hipSuccess) {
        (void)hipGetLastError();
        fhe_tlwe_pack_key_destroy(k);
        return FHE_ERR_HIP;
    }
    {
        StreamWs wsp(words * sizeof(u64), st);  // the residues of one prime, transformed in place
        rc = wsp.rc;
        u64 *tmp = wsp.as<u64>();
        for (int pi = 0; pi < 2 && rc == FHE_OK; ++pi) {
            rc = fhe::launch<fhe::torus_residue_kernel>(grid_for(words), 256, 0, st, (const u64 *)k->d_raw, tmp, words, pi ? t->T.p1 : t->T.p0);
            if (rc == FHE_OK) rc = fhe::ntt_fwd_multi(t->d_descs + pi, 1, tmp, log_n, polys, st, 60);
            if (rc == FHE_OK)
                rc = with_torus<TorusRing>(log_n, [&](auto wr) {
                    using W = typename decltype(wr)::type;
                    return fhe::launch<fhe::pack_key_permute_kernel<W>>(grid_for(words), 256, 0, st, (const u64 *)tmp, k->d_rows[pi], polys, 60);
                });
        }
    }
    // the key may serve calls on any stream from here on: wait for its rows
    if (hipStreamSynchronize(st) != hipSuccess && rc == FHE_OK) { (void)hipGetLastError(); rc = FHE_ERR_HIP; }
    if (rc != FHE_OK) { fhe_tlwe_pack_key_destroy(k); return rc; }
    *out = k;
    return FHE_OK;
}

// include/fhe_ring.h: the packing key switch
int fhe_tlwe_pack(const fhe_torus_ctx *t, const fhe_tlwe_pack_key *key, const uint64_t *ct_a, const uint64_t *ct_b, size_t count, size_t stride,
                  size_t packs, uint64_t *out_a, uint64_t *out_b, fhe_mem mem, void *stream) {
    if (!t || !key || key->t != t) return FHE_ERR_INVALID;
    const size_t n = size_t(1) << key->log_n;
    const int rc0 = fhe::pack_call_check(count, stride, n);
    if (rc0 != FHE_OK) return rc0;
    if ((!ct_a || !ct_b || !out_a || !out_b) && packs) return FHE_ERR_INVALID;
    if (packs && out_a == out_b) return FHE_ERR_INVALID;
    if (packs && mem == FHE_MEM_DEVICE && (out_a == ct_a || out_a == ct_b || out_b == ct_a || out_b == ct_b))
        return FHE_ERR_INVALID;  // the outputs are zeroed or written before every input is read
    if (packs == 0) return FHE_OK;
    if (packs > 0x7fffffffull / count) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    Mirror ma(ct_a, packs * count * key->n_in, mem, true, st), mb(ct_b, packs * count, mem, true, st), moa(out_a, packs * n, mem, false, st),
        mob(out_b, packs * n, mem, false, st);
    if (ma.rc | mb.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    int rc = pack_dev(key, ma.d, mb.d, count, stride, packs, moa.d, mob.d, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

}  // extern "C"
