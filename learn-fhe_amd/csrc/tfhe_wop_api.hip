// extern "C" entry points of the look-up without a padding bit (k = 1): a TLWE ciphertext of an m-bit message becomes m TGGSW selectors
// (fhe_tfhe_wop_selectors), and with a reserved selector key and a packed table, T[message] in one call (fhe_tfhe_wop_pbs).  Host logic
// in tfhe_wop.hpp; the new kernels in tfhe_wop_kernels.hpp; everything else goes through the public entries on device memory.
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "torus_ctx.hpp"
#include "dispatch.hpp"
#include "tfhe_lut.hpp"
#include "tfhe_wop.hpp"
#include "tfhe_wop_kernels.hpp"

namespace {

typedef uint64_t U;

struct WopArgs {
    const fhe_torus_ctx *t;
    const fhe_tggsw_key *brk;
    int ks_log_b, ks_d;
    const U *ksk_a, *ksk_b;  // as the caller gave them: checked for NULL here, read through the device pointers below
    int cb_log_b, cb_d, pf_log_b, pf_d;
    const U *pfksk;
    int m;
};

// the argument checks the two entries share (no pointer of the batch)
int wop_args_check(const WopArgs &A, size_t batch) {
    if (!A.t || !A.brk || A.brk->t != A.t || !A.pfksk) return FHE_ERR_INVALID;
    const size_t n = size_t(1) << A.brk->log_n;
    int rc = fhe::wop_check(A.cb_log_b, A.cb_d, n, A.m);
    if (rc != FHE_OK) return rc;
    if (A.m > 1) {  // a one-bit message needs no correction and so no key-switch key
        fhe::TDecomp KP;
        rc = make_tdecomp(A.ks_log_b, A.ks_d, &KP);
        if (rc != FHE_OK) return rc;
        if (!A.ksk_a || !A.ksk_b) return FHE_ERR_INVALID;
    }
    rc = fhe::wop_batch_check(A.m, A.cb_d, A.brk->count, batch);
    if (rc != FHE_OK) return rc;
    return fhe::pfks_check(A.pf_log_b, A.pf_d, 2, n, n, (size_t)A.cb_d, batch * A.m * A.cb_d);
}

// The m steps and the private functional key switch on device buffers.  ksk, pfksk, lwe, rows: device; rem_a / rem_b (device, or null):
// the running remainder lives there instead of in the workspace, and is rem_{m-1} when the loop ends.
int wop_selectors_dev(const WopArgs &A, const u64 *ksk_a, const u64 *ksk_b, const u64 *pfksk, const u64 *lwe_a, const u64 *lwe_b, u64 *rows_a,
                      u64 *rows_b, u64 *rem_a, u64 *rem_b, size_t batch, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const size_t n = size_t(1) << A.brk->log_n, n_lwe = A.brk->count;
    const int m = A.m, cb_d = A.cb_d, nu = fhe::wop_nu(cb_d), bits = 64 - (A.brk->log_n + 1);
    const fhe::WopScratch S(n, n_lwe, m, cb_d, batch);
    StreamWs wsp(S.total * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ws = wsp.as<u64>(), *ra = ws + S.L.acc_a, *rb = ws + S.L.acc_b, *ea = ws + S.L.ext_a, *eb = ws + S.L.ext_b, *at = ws + S.L.at, *bt = ws + S.L.bt;
    u64 *cxa = ws + S.cx_a, *cxb = ws + S.cx_b, *tab = ws + S.tab, *ca = ws + S.cor_a, *cb = ws + S.cor_b;
    if (!rem_a) { rem_a = ws + S.rem_a; rem_b = ws + S.rem_b; }
    int rc = fhe::launch<fhe::wop_tables_kernel>(grid_for(size_t(m) * n), 256, 0, st, tab, (unsigned)n, m, nu, A.cb_log_b, cb_d);
    for (int l = 0; l < m && rc == FHE_OK; ++l) {
        const bool last = l == m - 1;
        rc = fhe::launch<fhe::wop_front_kernel>(grid_for(batch * (n_lwe + 1)), 256, 0, st, l ? (const u64 *)rem_a : lwe_a, l ? (const u64 *)rem_b : lwe_b,
                                                l ? (const u64 *)ca : nullptr, l ? (const u64 *)cb : nullptr, rem_a, rem_b, batch * n_lwe, batch, m - 1 - l, bits,
                                                nu, at, bt);
        if (rc == FHE_OK)
            rc = fhe_tfhe_blind_rotate(A.t, A.brk, (const U *)at, (const U *)bt, (const U *)(tab + size_t(l) * n), (U *)ra, (U *)rb, batch, FHE_MEM_DEVICE, stream);
        if (rc == FHE_OK)
            rc = fhe::launch<fhe::wop_extract_kernel>(grid_for(batch * (cb_d + !last) * n), 256, 0, st, (const u64 *)ra, (const u64 *)rb, (unsigned)n,
                                                      (unsigned)batch, A.cb_log_b, cb_d, int(!last), fhe::wop_log_delta(m, l), size_t(m) * cb_d, size_t(l) * cb_d,
                                                      ea, eb, cxa, cxb);
        if (rc == FHE_OK && !last)
            rc = fhe_tlwe_key_switch(A.ks_log_b, A.ks_d, (const U *)ksk_a, (const U *)ksk_b, (const U *)cxa, (const U *)cxb, n, n_lwe, (U *)ca, (U *)cb, batch,
                                     FHE_MEM_DEVICE, stream);
    }
    if (rc == FHE_OK)
        rc = fhe_tlwe_pfks(A.pf_log_b, A.pf_d, (const U *)pfksk, 2, (const U *)ea, (const U *)eb, n, n, (size_t)cb_d, (U *)rows_a, (U *)rows_b,
                           batch * m * cb_d, FHE_MEM_DEVICE, stream);
    return rc;
}

}  // namespace

extern "C" {

int fhe_tfhe_wop_table(int cb_log_b, int cb_d, size_t n, int log_delta, uint64_t *out) { return fhe::wop_table(cb_log_b, cb_d, n, log_delta, out); }

int fhe_tfhe_wop_workspace(size_t n, size_t n_lwe, int m, int cb_d, size_t batch, size_t *words) {
    return fhe::wop_workspace(n, n_lwe, m, cb_d, batch, words);
}

// include/fhe_ring.h: the front of one step on its own
int fhe_tfhe_wop_front(const uint64_t *src_a, const uint64_t *src_b, const uint64_t *cor_a, const uint64_t *cor_b, size_t n_lwe, size_t batch, size_t n,
                       int nu, int shift, uint64_t *rem_a, uint64_t *rem_b, uint64_t *at, uint64_t *bt, fhe_mem mem, void *stream) {
    if (!is_pow2(n) || n < 2 || n_lwe == 0 || nu < 0 || nu > 5 || (n >> nu) == 0 || shift < 0 || shift > 63) return FHE_ERR_INVALID;
    if ((cor_a == nullptr) != (cor_b == nullptr) || ((!src_a || !src_b || !rem_a || !rem_b || !at || !bt) && batch)) return FHE_ERR_INVALID;
    if (batch && (at == bt || rem_a == rem_b || at == rem_a || at == rem_b || bt == rem_a || bt == rem_b)) return FHE_ERR_INVALID;
    if (batch > 0x7fffffffull / (n_lwe + 1)) return FHE_ERR_UNSUPPORTED;
    if (batch == 0) return FHE_OK;
    PtrDeviceGuard pguard(src_a, mem);
    if (!pguard.ok) return FHE_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    const size_t words = batch * n_lwe;
    Mirror ma(src_a, words, mem, true, st), mb(src_b, batch, mem, true, st), mca(cor_a, cor_a ? words : 0, mem, true, st), mcb(cor_b, cor_b ? batch : 0, mem, true, st),
        mra(rem_a, words, mem, false, st), mrb(rem_b, batch, mem, false, st), mta(at, words, mem, false, st), mtb(bt, batch, mem, false, st);
    if (ma.rc | mb.rc | mca.rc | mcb.rc | mra.rc | mrb.rc | mta.rc | mtb.rc) return FHE_ERR_HIP;
    FHE_TRY(fhe::launch<fhe::wop_front_kernel>(grid_for(words + batch), 256, 0, st, (const u64 *)ma.d, (const u64 *)mb.d, (const u64 *)mca.d, (const u64 *)mcb.d,
                                               mra.d, mrb.d, words, batch, shift, 64 - (ilog2(n) + 1), nu, mta.d, mtb.d));
    for (Mirror *m : {&mra, &mrb, &mta, &mtb}) FHE_TRY(m->sync_out(st));
    return FHE_OK;
}

// include/fhe_ring.h: an m-bit TLWE message -> m TGGSW selectors
int fhe_tfhe_wop_selectors(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a, const uint64_t *ksk_b,
                           int cb_log_b, int cb_d, int pf_log_b, int pf_d, const uint64_t *pfksk, int m, const uint64_t *lwe_a, const uint64_t *lwe_b,
                           uint64_t *rows_a, uint64_t *rows_b, uint64_t *rem_a, uint64_t *rem_b, size_t batch, fhe_mem mem, void *stream) {
    const WopArgs A{t, brk, ks_log_b, ks_d, ksk_a, ksk_b, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m};
    int rc = wop_args_check(A, batch);
    if (rc != FHE_OK) return rc;
    if (((!lwe_a || !lwe_b || !rows_a || !rows_b) && batch) || (rem_a == nullptr) != (rem_b == nullptr)) return FHE_ERR_INVALID;
    if (batch && (rows_a == rows_b || (rem_a && (rem_a == rem_b || rem_a == rows_a || rem_a == rows_b || rem_b == rows_a || rem_b == rows_b))))
        return FHE_ERR_INVALID;
    if (batch && mem == FHE_MEM_DEVICE)  // the outputs are written while the inputs and the keys are still read
        for (const uint64_t *o : {(const uint64_t *)rows_a, (const uint64_t *)rows_b, (const uint64_t *)rem_a, (const uint64_t *)rem_b})
            if (o && (o == lwe_a || o == lwe_b || o == pfksk || o == ksk_a || o == ksk_b)) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t n = size_t(1) << brk->log_n, n_lwe = brk->count, outs = batch * m * 2 * cb_d * n, ks_rows = m > 1 ? n * (size_t)ks_d : 0;
    Mirror mka(ksk_a, ks_rows * n_lwe, mem, true, st), mkb(ksk_b, ks_rows, mem, true, st), mk(pfksk, fhe::pfksk_words(pf_d, n, 2, n), mem, true, st),
        ma(lwe_a, n_lwe * batch, mem, true, st), mb(lwe_b, batch, mem, true, st), moa(rows_a, outs, mem, false, st), mob(rows_b, outs, mem, false, st),
        mra(rem_a, rem_a ? n_lwe * batch : 0, mem, false, st), mrb(rem_b, rem_b ? batch : 0, mem, false, st);
    if (mka.rc | mkb.rc | mk.rc | ma.rc | mb.rc | moa.rc | mob.rc | mra.rc | mrb.rc) return FHE_ERR_HIP;
    rc = wop_selectors_dev(A, mka.d, mkb.d, mk.d, ma.d, mb.d, moa.d, mob.d, mra.d, mrb.d, batch, stream);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    if (rc == FHE_OK) rc = mra.sync_out(st);
    if (rc == FHE_OK) rc = mrb.sync_out(st);
    return rc;
}

// include/fhe_ring.h: an m-bit TLWE message -> T[message] in one call
int fhe_tfhe_wop_pbs(const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a, const uint64_t *ksk_b, int cb_log_b,
                     int cb_d, int pf_log_b, int pf_d, const uint64_t *pfksk, int m, const uint64_t *lwe_a, const uint64_t *lwe_b, fhe_tggsw_key *sel_key,
                     size_t first_index, const uint64_t *polys, size_t n_out, int out_ks_log_b, int out_ks_d, const uint64_t *out_ksk_a,
                     const uint64_t *out_ksk_b, size_t n_lwe_out, uint64_t *out_a, uint64_t *out_b, size_t batch, fhe_mem mem, void *stream) {
    const WopArgs A{t, brk, ks_log_b, ks_d, ksk_a, ksk_b, cb_log_b, cb_d, pf_log_b, pf_d, pfksk, m};
    int rc = wop_args_check(A, batch);
    if (rc != FHE_OK) return rc;
    // the selector key: this context's, the step's ring, the circuit bootstrap's gadget
    if (!sel_key || sel_key->t != t || sel_key == brk || sel_key->log_n != brk->log_n || sel_key->log_b != cb_log_b || sel_key->d != cb_d) return FHE_ERR_INVALID;
    if (!polys || ((!lwe_a || !lwe_b || !out_a || !out_b) && batch)) return FHE_ERR_INVALID;
    const size_t n = size_t(1) << brk->log_n, n_lwe = brk->count;
    fhe::LutShape LS;
    rc = fhe::lut_shape(m, n_out, n, &LS);
    if (rc != FHE_OK) return rc;
    if (!fhe::lut_selectors_ok(first_index, batch, m, sel_key->count)) return FHE_ERR_INVALID;
    if ((out_ksk_a == nullptr) != (out_ksk_b == nullptr) || (out_ksk_a && n_lwe_out == 0)) return FHE_ERR_INVALID;
    if (batch && out_a == out_b) return FHE_ERR_INVALID;
    if (batch && mem == FHE_MEM_DEVICE)
        for (const uint64_t *o : {(const uint64_t *)out_a, (const uint64_t *)out_b})
            if (o == lwe_a || o == lwe_b || o == pfksk || o == ksk_a || o == ksk_b || o == polys || o == out_ksk_a || o == out_ksk_b) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t sel_words = batch * m * 2 * cb_d * n, ks_rows = m > 1 ? n * (size_t)ks_d : 0;
    // Everything below stays allocated until the look-up has been queued (host memory: has finished): a block released here would be
    // handed to the look-up's own host mirrors while the kernels that read it are still pending
    Mirror mka(ksk_a, ks_rows * n_lwe, mem, true, st), mkb(ksk_b, ks_rows, mem, true, st), mk(pfksk, fhe::pfksk_words(pf_d, n, 2, n), mem, true, st),
        ma(lwe_a, n_lwe * batch, mem, true, st), mb(lwe_b, batch, mem, true, st);
    if (mka.rc | mkb.rc | mk.rc | ma.rc | mb.rc) return FHE_ERR_HIP;
    StreamWs rows(2 * sel_words * sizeof(u64), st);  // the selectors' rows, a then b: read by the fill
    if (rows.rc != FHE_OK) return rows.rc;
    u64 *sa = rows.as<u64>(), *sb = sa + sel_words;
    rc = wop_selectors_dev(A, mka.d, mkb.d, mk.d, ma.d, mb.d, sa, sb, nullptr, nullptr, batch, stream);
    if (rc == FHE_OK) rc = fhe_tggsw_key_fill(sel_key, first_index, (const U *)sa, (const U *)sb, batch * m, FHE_MEM_DEVICE, stream);
    if (rc != FHE_OK) return rc;
    // host memory: the look-up copies its operands in from pageable memory next; let the queued work finish first (the call waits at its end anyway)
    if (mem != FHE_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(st));
    return fhe_tfhe_lut_eval(t, sel_key, first_index, m, polys, n_out, out_ks_log_b, out_ks_d, out_ksk_a, out_ksk_b, n_lwe_out, out_a, out_b, batch, mem, stream);
}

}  // extern "C"
