// extern "C" entry points of the TGLWE automorphism key switch (k = 1): the key set (generation, prepared form), the automorphism, the
// trace and the ring packing of TLWE ciphertexts.  include/fhe_ring.h has the definitions; tfhe_trace.hpp the rules that need no device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "torus_ctx.hpp"
#include "dispatch.hpp"
#include "torus_dispatch.hpp"
#include "tfhe_mul.hpp"
#include "tfhe_trace.hpp"
#include "tfhe_trace_kernels.hpp"
#include "tglwe_key_rows.hpp"

// A set of automorphism keys in the evaluation domain of the two 60-bit primes: per prime [n_g][d][2][n], key_perm layout.
struct fhe_tglwe_auto_key {
    const fhe_torus_ctx *t = nullptr;
    int device = -1;  // t's device, kept here: destroying the key must not read a context that may be gone already
    int log_n = 0;
    std::vector<unsigned> gs;
    u64 *d_rows[2] = {nullptr, nullptr};  // one allocation
    fhe::TDecomp P{};
};

namespace {

constexpr size_t RING_PACK_SLAB_BYTES = size_t(256) << 20;  // scratch of the packs one launch group works on (the tree's inner levels)

inline bool batch_fits(size_t batch) { return batch <= 0x7fffffffull; }

// [a, a + wa) and [b, b + wb) share a word
inline bool ranges_overlap(const uint64_t *a, size_t wa, const uint64_t *b, size_t wb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x < (uintptr_t)wa * sizeof(uint64_t) : x - y < (uintptr_t)wb * sizeof(uint64_t);
}

// every g odd and below 2n, none twice
bool gs_ok(const uint32_t *gs, size_t n_g, size_t n) {
    for (size_t i = 0; i < n_g; ++i) {
        if (!fhe::trace_g_ok(gs[i], n)) return false;
        for (size_t j = 0; j < i; ++j)
            if (gs[j] == gs[i]) return false;
    }
    return true;
}

// index of g in the key's set, -1 if it has none
int key_index(const fhe_tglwe_auto_key *key, unsigned g) {
    for (size_t i = 0; i < key->gs.size(); ++i)
        if (key->gs[i] == g) return (int)i;
    return -1;
}

size_t key_stride(const fhe_tglwe_auto_key *key) { return (size_t(2) * key->P.d) << key->log_n; }  // words of one key, one prime

fhe::RelinKeyArg key_arg(const fhe_tglwe_auto_key *key, int index) {
    const size_t off = size_t(index) * key_stride(key);
    return fhe::RelinKeyArg{key->d_rows[0] + off, key->d_rows[1] + off, key->t->T, key->P};
}

// the table of the steps u = hi .. lo + 1; false if the set lacks one of their keys
bool trace_keys(const fhe_tglwe_auto_key *key, int lo, int hi, fhe::TraceKeysArg *K) {
    K->steps = 0;
    K->T = key->t->T;
    K->P = key->P;
    for (int s = 0; s < fhe::TRACE_MAX_STEPS; ++s) { K->rows0[s] = K->rows1[s] = nullptr; K->g[s] = 1; }
    for (int u = hi; u > lo; --u) {
        const unsigned g = fhe::trace_g(u);
        const int q = key_index(key, g);
        if (q < 0) return false;
        const fhe::RelinKeyArg a = key_arg(key, q);
        K->rows0[K->steps] = a.rows0; K->rows1[K->steps] = a.rows1; K->g[K->steps] = g;
        ++K->steps;
    }
    return true;
}

template <class W>
unsigned team_blocks(size_t teams) { return (unsigned)((teams + W::TEAMS - 1) / W::TEAMS); }

int trace_dev(const fhe_tglwe_auto_key *key, const fhe::TraceKeysArg &K, const u64 *in_a, const u64 *in_b, bool keep, bool embed, u64 *out_a, u64 *out_b,
              size_t batch, hipStream_t st) {
    return with_torus<TorusRing>(key->log_n, [&](auto wr) {
        using W = typename decltype(wr)::type;
        return fhe::launch<fhe::tglwe_trace_kernel<W>>(team_blocks<W>(batch), W::THREADS, W::TORUS_LDS_BYTES, st, K, in_a, in_b, keep ? 1u : 0u, embed ? 1u : 0u,
                                                       out_a, out_b, (unsigned)batch);
    });
}

int merge_dev(const fhe_tglwe_auto_key *key, int index, const fhe::PackLevel &L, const u64 *in_a, const u64 *in_b, bool embed, u64 *out_a, u64 *out_b,
              size_t teams, hipStream_t st) {
    return with_torus<TorusRing>(key->log_n, [&](auto wr) {
        using W = typename decltype(wr)::type;
        return fhe::launch<fhe::tglwe_merge_kernel<W>>(team_blocks<W>(teams), W::THREADS, W::TORUS_LDS_BYTES, st, key_arg(key, index), in_a, in_b, L.g, L.rot,
                                                       L.nodes, embed ? 1u : 0u, out_a, out_b, (unsigned)teams);
    });
}

// packs on device buffers: the tree level by level, the last level into out, then the trace in place
int ring_pack_dev(const fhe_tglwe_auto_key *key, const fhe::TraceKeysArg &K, const int *level_key, int c, const u64 *ct_a, const u64 *ct_b, size_t packs,
                  u64 *out_a, u64 *out_b, hipStream_t st) {
    const int log_n = key->log_n;
    const size_t n = size_t(1) << log_n, count = size_t(1) << c;
    if (c == 0) return trace_dev(key, K, ct_a, ct_b, true, true, out_a, out_b, packs, st);
    const size_t per_pack = fhe::pack_scratch_words(c, log_n) * sizeof(u64);
    const size_t slab = fhe::ring_pack_slab(packs, per_pack, RING_PACK_SLAB_BYTES, count / 2, 0x7fffffffull, fhe::opt(fhe::OPT_PACK_SLAB));
    StreamWs wsp(slab * per_pack, st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    for (size_t g0 = 0; g0 < packs; g0 += slab) {
        const size_t gs = std::min(slab, packs - g0);
        // buffer 0: gs count / 2 ciphertexts (a halves, then b halves), buffer 1: gs count / 4
        u64 *buf_a[2], *buf_b[2];
        buf_a[0] = wsp.as<u64>();
        buf_b[0] = buf_a[0] + gs * (count / 2) * n;
        buf_a[1] = buf_b[0] + gs * (count / 2) * n;
        buf_b[1] = buf_a[1] + gs * (count / 4) * n;
        const u64 *in_a = ct_a + g0 * count * n, *in_b = ct_b + g0 * count;
        for (int v = 1; v <= c; ++v) {
            const fhe::PackLevel L = fhe::pack_level(v, c, log_n);
            u64 *oa = v == c ? out_a + g0 * n : buf_a[(v - 1) & 1], *ob = v == c ? out_b + g0 * n : buf_b[(v - 1) & 1];
            FHE_TRY(merge_dev(key, level_key[v], L, in_a, in_b, v == 1, oa, ob, gs * L.nodes, st));
            in_a = oa;
            in_b = ob;
        }
    }
    if (K.steps > 0) return trace_dev(key, K, out_a, out_b, true, false, out_a, out_b, packs, st);
    return FHE_OK;
}

}  // namespace

extern "C" {

// include/fhe_ring.h: the rows -h_j sigma_g(S) on the device, then fhe_tglwe_sk_encrypt on them
int fhe_tglwe_atk_gen(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *sk, size_t n, const uint32_t *gs, size_t n_g, double std_dev,
                      const fhe_rng *rng, uint64_t stream_id, uint64_t *atk_a, uint64_t *atk_b, fhe_mem mem, void *stream) {
    if (!t || !sk || !gs || !rng || !atk_a || !atk_b || !(std_dev >= 0)) return FHE_ERR_INVALID;
    const int rc0 = fhe::mul_gadget_check(log_b, d, n);
    if (rc0 != FHE_OK) return rc0;
    if (n_g < 1 || n_g > n || !gs_ok(gs, n_g, n)) return FHE_ERR_INVALID;
    if (t->device < 0) return FHE_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t rows = n_g * size_t(d), words = rows * n;
    Mirror msk(sk, n, mem, true, st), ma(atk_a, words, mem, false, st), mb(atk_b, words, mem, false, st);
    if (msk.rc | ma.rc | mb.rc) return FHE_ERR_HIP;
    StreamWs wsp(words * sizeof(u64), st), wsg(n_g * sizeof(uint32_t), st);  // the plaintext rows; the Galois elements
    if (wsp.rc != FHE_OK) return wsp.rc;
    if (wsg.rc != FHE_OK) return wsg.rc;
    // gs is the caller's host array whatever `mem` says (a parameter list, like log_b and d); pageable memory: the copy has left it when the call returns
    HIP_TRY(hipMemcpyAsync(wsg.p, gs, n_g * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FHE_TRY(fhe::launch<fhe::atk_plain_kernel>(grid_for(n_g * n), 256, 0, st, (const u64 *)msk.d, (unsigned)n, fhe::trace_log_n(n), (const unsigned *)wsg.p,
                                               (unsigned)n_g, log_b, d, wsp.as<u64>()));
    int rc = fhe_tglwe_sk_encrypt(t, (const uint64_t *)msk.d, (const uint64_t *)wsp.as<u64>(), n, rows, std_dev, rng, stream_id, (uint64_t *)ma.d,
                                  (uint64_t *)mb.d, FHE_MEM_DEVICE, stream);
    if (rc == FHE_OK) rc = ma.sync_out(st);
    if (rc == FHE_OK) rc = mb.sync_out(st);
    return rc;
}

void fhe_tglwe_atk_destroy(fhe_tglwe_auto_key *key) {
    if (!key) return;
    if (key->device >= 0 && key->d_rows[0]) {
        DeviceGuard guard(key->device);
        (void)hipFree(key->d_rows[0]);
    }
    delete key;
}

// include/fhe_ring.h: the n_g d rows, once, into the evaluation domain of the two 60-bit primes (the relinearisation key's transform)
int fhe_tglwe_atk_prepare(const fhe_torus_ctx *t, int log_b, int d, const uint64_t *atk_a, const uint64_t *atk_b, size_t n, const uint32_t *gs, size_t n_g,
                          fhe_mem mem, void *stream, fhe_tglwe_auto_key **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!t || !atk_a || !atk_b || !gs) return FHE_ERR_INVALID;
    int rc = fhe::mul_gadget_check(log_b, d, n);
    if (rc != FHE_OK) return rc;
    if (n_g < 1 || n_g > n || !gs_ok(gs, n_g, n)) return FHE_ERR_INVALID;
    fhe::TDecomp P;
    rc = make_tdecomp(log_b, d, &P);
    if (rc != FHE_OK) return rc;
    if (t->device < 0) return FHE_ERR_NO_DEVICE;
    const int log_n = fhe::trace_log_n(n);
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t rows = n_g * size_t(d), half = rows * n, words = 2 * half;  // of one prime
    fhe_tglwe_auto_key *k = new (std::nothrow) fhe_tglwe_auto_key();
    if (!k) return FHE_ERR_INVALID;
    k->t = t; k->device = t->device; k->log_n = log_n; k->P = P;
    k->gs.assign(gs, gs + n_g);
    if (hipMalloc((void **)&k->d_rows[0], 2 * words * sizeof(u64)) != hipSuccess) { (void)hipGetLastError(); delete k; return FHE_ERR_HIP; }
    k->d_rows[1] = k->d_rows[0] + words;
    {
        Mirror ma(atk_a, half, mem, true, st), mb(atk_b, half, mem, true, st);
        rc = (ma.rc | mb.rc) ? FHE_ERR_HIP : tglwe_rows_prepare(t, log_n, ma.d, mb.d, rows, k->d_rows, st);
        // the key may serve calls on any stream from here on: wait for its rows (and, with them, for the staging copies)
        if (hipStreamSynchronize(st) != hipSuccess && rc == FHE_OK) { (void)hipGetLastError(); rc = FHE_ERR_HIP; }
    }
    if (rc != FHE_OK) { fhe_tglwe_atk_destroy(k); return rc; }
    *out = k;
    return FHE_OK;
}

// include/fhe_ring.h: autks_g, one launch
int fhe_tglwe_automorphism(const fhe_torus_ctx *t, const fhe_tglwe_auto_key *key, uint32_t g, const uint64_t *ct_a, const uint64_t *ct_b, uint64_t *out_a,
                           uint64_t *out_b, size_t batch, fhe_mem mem, void *stream) {
    if (!t || !key || key->t != t || !ct_a || !ct_b || !out_a || !out_b) return FHE_ERR_INVALID;
    const size_t n = size_t(1) << key->log_n;
    if (!fhe::trace_g_ok(g, n)) return FHE_ERR_INVALID;
    const int q = key_index(key, g);
    if (q < 0) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!batch_fits(batch)) return FHE_ERR_UNSUPPORTED;
    const size_t words = batch * n;
    // out is the input, half for half, or overlaps nothing
    if (ranges_overlap(out_a, words, out_b, words) || ranges_overlap(ct_a, words, ct_b, words)) return FHE_ERR_INVALID;
    if ((out_a != ct_a && ranges_overlap(out_a, words, ct_a, words)) || (out_b != ct_b && ranges_overlap(out_b, words, ct_b, words)) ||
        ranges_overlap(out_a, words, ct_b, words) || ranges_overlap(out_b, words, ct_a, words))
        return FHE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    Mirror ma(ct_a, words, mem, true, st), mb(ct_b, words, mem, true, st), moa(out_a, words, mem, false, st), mob(out_b, words, mem, false, st);
    if (ma.rc | mb.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    fhe::TraceKeysArg K;
    (void)trace_keys(key, 0, 0, &K);
    const fhe::RelinKeyArg a = key_arg(key, q);
    K.rows0[0] = a.rows0; K.rows1[0] = a.rows1; K.g[0] = g; K.steps = 1;
    int rc = trace_dev(key, K, ma.d, mb.d, false, false, moa.d, mob.d, batch, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

// include/fhe_ring.h: the steps u = hi .. lo + 1 in one launch
int fhe_tglwe_trace(const fhe_torus_ctx *t, const fhe_tglwe_auto_key *key, int lo, int hi, const uint64_t *ct_a, const uint64_t *ct_b, uint64_t *out_a,
                    uint64_t *out_b, size_t batch, fhe_mem mem, void *stream) {
    if (!t || !key || key->t != t || !ct_a || !ct_b || !out_a || !out_b) return FHE_ERR_INVALID;
    const size_t n = size_t(1) << key->log_n;
    if (!fhe::trace_range_ok(lo, hi, key->log_n)) return FHE_ERR_INVALID;
    fhe::TraceKeysArg K;
    if (!trace_keys(key, lo, hi, &K)) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    if (!batch_fits(batch)) return FHE_ERR_UNSUPPORTED;
    const size_t words = batch * n;
    if (ranges_overlap(out_a, words, out_b, words) || ranges_overlap(ct_a, words, ct_b, words)) return FHE_ERR_INVALID;
    if ((out_a != ct_a && ranges_overlap(out_a, words, ct_a, words)) || (out_b != ct_b && ranges_overlap(out_b, words, ct_b, words)) ||
        ranges_overlap(out_a, words, ct_b, words) || ranges_overlap(out_b, words, ct_a, words))
        return FHE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    Mirror ma(ct_a, words, mem, true, st), mb(ct_b, words, mem, true, st), moa(out_a, words, mem, false, st), mob(out_b, words, mem, false, st);
    if (ma.rc | mb.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    int rc = trace_dev(key, K, ma.d, mb.d, true, false, moa.d, mob.d, batch, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

// include/fhe_ring.h: the packing tree, one launch a level, and the trace
int fhe_tlwe_ring_pack(const fhe_torus_ctx *t, const fhe_tglwe_auto_key *key, const uint64_t *ct_a, const uint64_t *ct_b, size_t count, size_t packs,
                       uint64_t *out_a, uint64_t *out_b, fhe_mem mem, void *stream) {
    if (!t || !key || key->t != t || !ct_a || !ct_b || !out_a || !out_b) return FHE_ERR_INVALID;
    const int log_n = key->log_n;
    const size_t n = size_t(1) << log_n;
    const int c = fhe::pack_log_count(count, log_n);
    if (c < 0) return FHE_ERR_INVALID;
    // the keys of the levels l = 2 .. count and of the trace steps u = log2 n .. c + 1
    int level_key[fhe::TRACE_MAX_STEPS + 1] = {0};
    for (int v = 1; v <= c; ++v) {
        level_key[v] = key_index(key, fhe::trace_g(v));
        if (level_key[v] < 0) return FHE_ERR_INVALID;
    }
    fhe::TraceKeysArg K;
    if (!trace_keys(key, c, log_n, &K)) return FHE_ERR_INVALID;
    if (packs == 0) return FHE_OK;
    if (packs > 0x7fffffffull / count) return FHE_ERR_UNSUPPORTED;
    {  // the levels and the trace write out while inputs are still to be read: no output may overlap an input or the other output
        const size_t wa = packs * count * n, wb = packs * count, wo = packs * n;
        if (ranges_overlap(out_a, wo, out_b, wo) || ranges_overlap(out_a, wo, ct_a, wa) || ranges_overlap(out_a, wo, ct_b, wb) ||
            ranges_overlap(out_b, wo, ct_a, wa) || ranges_overlap(out_b, wo, ct_b, wb))
            return FHE_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    Mirror ma(ct_a, packs * count * n, mem, true, st), mb(ct_b, packs * count, mem, true, st), moa(out_a, packs * n, mem, false, st),
        mob(out_b, packs * n, mem, false, st);
    if (ma.rc | mb.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    int rc = ring_pack_dev(key, K, level_key, c, ma.d, mb.d, packs, moa.d, mob.d, st);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

}  // extern "C"
