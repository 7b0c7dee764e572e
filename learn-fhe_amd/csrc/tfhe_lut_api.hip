// extern "C" entry points of the encrypted table look-up with vertical packing (k = 1): shape, packing and workspace on the host
// (tfhe_lut.hpp), and fhe_tfhe_lut_eval: CMUX-tree levels, the rotation ladder, extraction and the optional key switch as one call in
// which every ciphertext uses its own selectors.
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "torus_ctx.hpp"
#include "dispatch.hpp"
#include "torus_dispatch.hpp"
#include "tfhe_lut.hpp"
#include "tfhe_lut_kernels.hpp"

namespace {

// the library's rule for LUT_EXTRACT = 0: the ladder writes the extractions itself
constexpr bool LUT_RULE_FUSED = true;

// One tree level (polys or in_* -> out_*) under the key's form.  The key argument starts at the call's first selector; the kernels add
// (c m + l) entries.
int launch_lut_level(const fhe_torus_ctx *t, const fhe_tggsw_key *key, size_t first_index, const u64 *polys, const u64 *in_a, const u64 *in_b, u64 *out_a,
                     u64 *out_b, const fhe::LutJobs &J, hipStream_t st) {
    return with_key_form<false>(t, key, first_index, [&](auto form, auto k, size_t lds) {
        using Form = typename decltype(form)::type;
        return fhe::launch_teams<fhe::tfhe_lut_level_kernel<Form>, typename Form::Ring>(J.jobs, lds, st, polys, in_a, in_b, out_a, out_b, J, k);
    });
}

// The rotation ladder on acc; ext_a != null: it writes the extractions (ext_a [batch n_out][n], ext_b [batch n_out]) instead of storing
// the accumulators; polys != null: there was no tree, the accumulators start from the shared polynomials
int launch_lut_ladder(const fhe_torus_ctx *t, const fhe_tggsw_key *key, size_t first_index, const u64 *polys, u64 *acc_a, u64 *acc_b, u64 *ext_a, u64 *ext_b,
                      const fhe::LutJobs &J, hipStream_t st) {
    return with_key_form<true>(t, key, first_index, [&](auto form, auto k, size_t lds) {
        using Form = typename decltype(form)::type;
        return fhe::with_bool(polys != nullptr, [&](auto fp) {
            return fhe::launch_teams<fhe::tfhe_lut_ladder_kernel<Form, decltype(fp)::value>, typename Form::Ring>(J.jobs, lds, st, polys, acc_a, acc_b, ext_a,
                                                                                                                ext_b, J, k);
        });
    });
}

}  // namespace

extern "C" {

int fhe_tfhe_lut_shape(int m, size_t n_out, size_t n, int *r, size_t *per_acc, size_t *n_acc, size_t *n_polys) {
    fhe::LutShape S;
    const int rc = fhe::lut_shape(m, n_out, n, &S);
    if (rc != FHE_OK) return rc;
    if (r) *r = S.r;
    if (per_acc) *per_acc = S.per_acc;
    if (n_acc) *n_acc = S.n_acc;
    if (n_polys) *n_polys = S.n_polys;
    return FHE_OK;
}

int fhe_tfhe_lut_pack(const uint64_t *table, int m, size_t n_out, size_t n, uint64_t *polys) { return fhe::lut_pack(table, m, n_out, n, polys); }

int fhe_tfhe_lut_workspace(size_t n, int m, size_t n_out, size_t n_lwe_out, size_t batch, size_t *words) {
    return fhe::lut_workspace(n, m, n_out, n_lwe_out, batch, words);
}

// include/fhe_ring.h: the look-up in one call
int fhe_tfhe_lut_eval(const fhe_torus_ctx *t, const fhe_tggsw_key *sel_key, size_t first_index, int m, const uint64_t *polys, size_t n_out, int ks_log_b,
                      int ks_d, const uint64_t *ksk_a, const uint64_t *ksk_b, size_t n_lwe_out, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem,
                      void *stream) {
    if (!t || !sel_key || sel_key->t != t || !polys || ((!out_a || !out_b) && batch)) return FHE_ERR_INVALID;
    const size_t n = size_t(1) << sel_key->log_n;
    fhe::LutShape S;
    int rc = fhe::lut_shape(m, n_out, n, &S);
    if (rc != FHE_OK) return rc;
    const bool ks = ksk_a != nullptr;
    if (ks) {
        fhe::TDecomp KP;
        rc = make_tdecomp(ks_log_b, ks_d, &KP);
        if (rc != FHE_OK) return rc;
        if (!ksk_b || n_lwe_out == 0) return FHE_ERR_INVALID;
    } else if (ksk_b) {
        return FHE_ERR_INVALID;
    }
    if (!fhe::lut_selectors_ok(first_index, batch, m, sel_key->count)) return FHE_ERR_INVALID;
    rc = fhe::lut_batch_check(S, batch);
    if (rc != FHE_OK) return rc;
    if (batch && out_a == out_b) return FHE_ERR_INVALID;
    if (batch && mem == FHE_MEM_DEVICE)  // the outputs are written before every ciphertext has read the shared inputs
        for (const uint64_t *o : {(const uint64_t *)out_a, (const uint64_t *)out_b})
            if (o == polys || o == ksk_a || o == ksk_b) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t width = ks ? n_lwe_out : n, rows = batch * n_out, ks_rows = ks ? n * (size_t)ks_d : 0;
    Mirror mp(polys, S.n_polys * n, mem, true, st), mka(ksk_a, ks_rows * n_lwe_out, mem, true, st), mkb(ksk_b, ks_rows, mem, true, st),
        moa(out_a, rows * width, mem, false, st), mob(out_b, rows, mem, false, st);
    if (mp.rc | mka.rc | mkb.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    const fhe::TfheScratch L = fhe::lut_scratch(S, ks ? n_lwe_out : 0, batch);
    StreamWs wsp(L.total * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ws = wsp.as<u64>(), *na = ws + L.acc_a, *nb = ws + L.acc_b;
    const size_t accs = batch * S.n_acc;
    fhe::LutJobs J{};
    J.n_acc = (unsigned)S.n_acc;
    J.m = (unsigned)m;
    J.log_polys = (unsigned)S.h;
    // the tree over the high bits: level v halves the nodes, alternating between the two areas (tfhe_lut.hpp)
    for (int v = 0; v < S.h && rc == FHE_OK; ++v) {
        const size_t half = size_t(1) << (S.h - 1 - v);
        const size_t src = v ? fhe::lut_level_area(S.h, v - 1, accs) * n : 0, dst = fhe::lut_level_area(S.h, v, accs) * n;
        J.jobs = (unsigned)(accs * half);
        J.half = (unsigned)half;
        J.first = (unsigned)(S.r + v);
        rc = launch_lut_level(t, sel_key, first_index, v ? nullptr : (const u64 *)mp.d, na + src, nb + src, na + dst, nb + dst, J, st);
    }
    // the rotation by the low bits, then the extractions
    u64 *acc_a = na + fhe::lut_acc_area(S.h, accs) * n, *acc_b = nb + fhe::lut_acc_area(S.h, accs) * n;
    J.jobs = (unsigned)accs;
    J.half = 1;
    J.first = 0;
    J.steps = (unsigned)S.r;
    u64 *ea = ks ? ws + L.ext_a : moa.d, *eb = ks ? ws + L.ext_b : mob.d;
    int log_per = 0;
    while ((size_t(1) << log_per) < S.per_acc) ++log_per;
    J.n_out = (unsigned)n_out;
    J.log_per = (unsigned)log_per;
    // who extracts (DESIGN.md 9.4 has the measurement behind the rule; lab switch LUT_EXTRACT: 1 the ladder, 2 the kernel): the same bits
    const long lab_extract = fhe::opt(fhe::OPT_LUT_EXTRACT);
    const bool fused = lab_extract == 1 || (lab_extract != 2 && LUT_RULE_FUSED);
    if (rc == FHE_OK)
        rc = launch_lut_ladder(t, sel_key, first_index, S.h ? nullptr : (const u64 *)mp.d, acc_a, acc_b, fused ? ea : nullptr, fused ? eb : nullptr, J, st);
    if (rc == FHE_OK && !fused)
        rc = fhe::launch<fhe::tfhe_lut_extract_kernel>(grid_for(rows * n), 256, 0, st, (const u64 *)acc_a, (const u64 *)acc_b, (unsigned)n, (unsigned)m,
                                                       (unsigned)log_per, (unsigned)S.n_acc, (unsigned)n_out, rows, ea, eb);
    typedef uint64_t U;
    if (rc == FHE_OK && ks)
        rc = fhe_tlwe_key_switch(ks_log_b, ks_d, (const U *)mka.d, (const U *)mkb.d, (const U *)ea, (const U *)eb, n, n_lwe_out, (U *)moa.d, (U *)mob.d, rows,
                                 FHE_MEM_DEVICE, stream);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

}  // extern "C"
