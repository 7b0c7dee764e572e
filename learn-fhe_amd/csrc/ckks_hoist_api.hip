// extern "C" entry points of the hoisted CKKS rotations: sigma_t in the evaluation domain (fhe_rns_automorphism_eval), R rotations of
// one ciphertext from ONE base extension and ONE set of forward transforms (fhe_ckks_rotate_many, single hoisting) and the diagonal-
// matrix product whose baby-step sums stay in qs || ps until each giant step divides by P once (fhe_ckks_mul_mat_hoisted, double
// hoisting).  include/fhe_ring.h has the definitions, ckks_hoist.hpp the index logic, ckks_hoist_kernels.hpp the kernels and the
// reduction schedule, DESIGN.md 4.13 the transform counts and the measurements.
//
// These entries extend BEFORE the automorphism, the reference's `rotate` after it: they are not the bits of `Ckks::rotate` /
// `Bootstrapping::mul_mat` (fhe_ckks_rotate and fhe_ckks_mul_mat are, and stay as they were).
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "api_common.hpp"
#include "ctx.hpp"
#include "dispatch.hpp"
#include "rns_ctx.hpp"
#include "rns_kernels.hpp"
#include "ckks_matmul_kernels.hpp"
#include "ckks_hoist.hpp"
#include "ckks_hoist_kernels.hpp"

struct fhe_ckks_diag_matrix_hoisted {
    const fhe_rns_ctx *hi = nullptr, *lo = nullptr;
    int device = -1;                       // hi->device, kept so that destroy does not read the (borrowed) context
    int log_n = 0, n_giant = 0, n_baby = 0, terms = 0;
    int max_terms = 0;                     // the longest giant step
    int fold = 0;                          // hoist_fold_bound of the widest of all L + K moduli
    std::vector<unsigned> t_giant;         // 5^i mod 2n (0 where i == 0: no rotation)
    std::vector<const fhe_ckks_key *> baby_keys, giant_keys;  // borrowed
    u64 *d_diag = nullptr;                 // [terms][L + K][n], evaluation domain
    // one allocation: kb [n_baby] | ka [n_baby] | red_mu [L + K] (8 bytes each) | term_start [n_giant + 1] | term_baby [terms] |
    // t_baby [n_baby] (4 bytes each)
    void *d_tab = nullptr;
    const u64 *const *d_kb = nullptr, *const *d_ka = nullptr;
    const u64 *d_mu = nullptr;
    const int *d_terms = nullptr;
    const unsigned *d_t = nullptr;
};

namespace {
// `CkksParam::pow5` (ckks.rs:49-51): 5^j mod 2n
unsigned pow5(uint32_t j, size_t n) {
    const uint64_t m = 2 * (uint64_t)n;
    uint64_t r = 1 % m, b = 5 % m;
    for (; j; j >>= 1, b = b * b % m)
        if (j & 1) r = r * b % m;
    return (unsigned)r;
}
// x over pairs of points, y over `rows` polynomials
dim3 pair_grid(size_t n, size_t rows) {
    const size_t gx = (n / 2 + 255) / 256;
    return dim3((unsigned)(gx > 64 ? 64 : gx), (unsigned)(rows > 65535 ? 65535 : rows));
}
// x over the points of one polynomial, one per thread, y over `rows` polynomials
dim3 coeff_grid(size_t n, size_t rows) {
    const size_t gx = (n + 255) / 256;
    return dim3((unsigned)(gx > 64 ? 64 : gx), (unsigned)(rows > 65535 ? 65535 : rows));
}
// the lift of one ciphertext batch: ext [batch][L+K][n] = ntt(a || ext(a)), bh [batch][L][n] = ntt(P b): one extension, 2 L + K
// forward transforms
int hoist_lift(const fhe_rns_ctx *r, const u64 *ct_b, const u64 *ct_a, u64 *ext, u64 *bh, int log_n, size_t batch, hipStream_t st) {
    const size_t n = size_t(1) << log_n, L = r->L, lk = size_t(r->L + r->K);
    FHE_TRY(fhe::ckks_extend_dev(r, ct_a, ext, n, batch, st));
    FHE_TRY(fhe::launch<fhe::ckks_hoist_scale_kernel>(coeff_grid(n, batch * L), 256, 0, st, ct_b, bh, (unsigned)n, (unsigned)L, batch * L, r->resc.half_q,
                                                      (const fhe::Barrett *)r->d_barrett));
    FHE_TRY(fhe::ntt_fwd_multi(r->d_descs, (unsigned)lk, ext, log_n, batch * lk, st, r->all_pm));
    return fhe::ntt_fwd_multi(r->d_descs, (unsigned)L, bh, log_n, batch * L, st, r->all_pm);
}
}  // namespace

extern "C" {

int fhe_rns_automorphism_eval(const fhe_rns_ctx *r, int extended, int64_t t, const uint64_t *in, uint64_t *out, size_t n, size_t batch, fhe_mem mem,
                              void *stream) {
    if (!r || !is_pow2(n) || (n >> 30) || ((!in || !out) && batch) || in == out) return FHE_ERR_INVALID;
    if (r->device < 0) return FHE_ERR_NO_DEVICE;
    const unsigned tt = rem_euclid_2n(t, n);
    if (!(tt & 1) && n > 1) return FHE_ERR_UNSUPPORTED;  // an even t is not a permutation of the evaluation points
    if (batch == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t limbs = size_t(extended ? r->L + r->K : r->L);
    if (batch >= fhe::HOIST_MAX_ROWS / limbs) return FHE_ERR_UNSUPPORTED;
    Mirror mi(in, n * batch * limbs, mem, true, st), mo(out, n * batch * limbs, mem, false, st);
    if (mi.rc | mo.rc) return FHE_ERR_HIP;
    FHE_TRY(fhe::launch<fhe::rns_automorphism_eval_kernel>(coeff_grid(n, batch * limbs), 256, 0, st, (const u64 *)mi.d, mo.d, ilog2(n), batch * limbs, tt));
    return mo.sync_out(st);
}

int fhe_ckks_rotate_many(const fhe_rns_ctx *r, size_t n, const uint32_t *amounts, const fhe_ckks_key *const *keys, int count, const uint64_t *ct_b,
                         const uint64_t *ct_a, uint64_t *const *out_b, uint64_t *const *out_a, size_t batch, fhe_mem mem, void *stream) {
    if (!r || count < 0 || (count && (!amounts || !keys || !out_b || !out_a))) return FHE_ERR_INVALID;
    int rc = fhe::ckks_ring_status(r, n);
    if (rc != FHE_OK) return rc;
    const int log_n = ilog2(n);
    for (int i = 0; i < count; ++i) {
        const fhe_ckks_key *k = keys[i];
        if (amounts[i] != 0 && !k) return FHE_ERR_INVALID;              // a rotation without its key
        if (k && (k->rns != r || k->log_n != log_n)) return FHE_ERR_INVALID;  // a key of another context or ring
        if (batch && (!out_b[i] || !out_a[i])) return FHE_ERR_INVALID;
    }
    if ((!ct_b || !ct_a) && batch && count) return FHE_ERR_INVALID;
    if (batch == 0 || count == 0) return FHE_OK;
    const size_t L = r->L, K = r->K, lk = L + K, in_w = batch * L * n;
    fhe::HoistRotWs lay;
    if (!fhe::hoist_rot_ws(n, L, K, batch, &lay)) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    Mirror mb(ct_b, in_w, mem, true, st), ma(ct_a, in_w, mem, true, st);
    if (mb.rc | ma.rc) return FHE_ERR_HIP;
    StreamWs wsp(lay.total * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ws = wsp.as<u64>(), *ext = ws + lay.ext, *bh = ws + lay.bh, *p = ws + lay.p;
    bool lifted = false;
    for (int i = 0; i < count; ++i) {
        Mirror mob(out_b[i], in_w, mem, false, st), moa(out_a[i], in_w, mem, false, st);
        if (mob.rc | moa.rc) return FHE_ERR_HIP;
        const fhe_ckks_key *k = keys[i];
        const unsigned t = pow5(amounts[i], n);
        if (amounts[i] == 0) {  // u_0 = (P b, P a): the division by P gives the ciphertext back
            HIP_TRY(hipMemcpyAsync(mob.d, mb.d, in_w * sizeof(u64), hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(moa.d, ma.d, in_w * sizeof(u64), hipMemcpyDeviceToDevice, st));
        } else {
            if (!lifted) FHE_TRY(hoist_lift(r, mb.d, ma.d, ext, bh, log_n, batch, st));
            lifted = true;
            FHE_TRY(fhe::launch<fhe::ckks_hoist_rot_kernel>(pair_grid(n, 2 * batch * lk), 256, 0, st, (const u64 *)ext, (const u64 *)bh, (const u64 *)k->d_kb,
                                                            (const u64 *)k->d_ka, p, t, log_n, (unsigned)L, (unsigned)lk, batch, 2 * batch * lk, r->resc.half_q,
                                                            (const fhe::Barrett *)r->d_barrett));
            FHE_TRY(fhe::ntt_inv_multi(r->d_descs, (unsigned)lk, p, log_n, 2 * batch * lk, st, r->all_pm));
            FHE_TRY(fhe::ckks_rescale_k_dev(r, p, mob.d, n, batch, st));
            FHE_TRY(fhe::ckks_rescale_k_dev(r, p + batch * lk * n, moa.d, n, batch, st));
        }
        rc = mob.sync_out(st);
        if (rc == FHE_OK) rc = moa.sync_out(st);
        if (rc != FHE_OK) return rc;
    }
    return FHE_OK;
}

void fhe_ckks_diag_matrix_hoisted_destroy(fhe_ckks_diag_matrix_hoisted *m) {
    if (!m) return;
    if (m->device >= 0) {
        DeviceGuard guard(m->device);
        if (m->d_diag) (void)hipFree(m->d_diag);
        if (m->d_tab) (void)hipFree(m->d_tab);
    }
    delete m;
}

int fhe_ckks_diag_matrix_prepare_hoisted(const fhe_rns_ctx *rns_hi, const fhe_rns_ctx *rns_lo, size_t n, const uint32_t *giant, int n_giant,
                                         const uint32_t *baby, int n_baby, const uint8_t *present, const uint64_t *diags,
                                         const fhe_ckks_key *const *baby_keys, const fhe_ckks_key *const *giant_keys, fhe_mem mem,
                                         fhe_ckks_diag_matrix_hoisted **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!rns_hi || !rns_lo) return FHE_ERR_INVALID;
    int rc = fhe::ckks_ring_status(rns_hi, n);
    if (rc != FHE_OK) return rc;
    const int L = rns_hi->L, lk = rns_hi->L + rns_hi->K;
    if (L < 2) return FHE_ERR_INVALID;  // the closing rescale would leave no limb
    // rns_lo: the prefix qs[0 .. L-1) with the same ps on the same device
    if (rns_lo->L != L - 1 || rns_lo->K != rns_hi->K || rns_lo->device != rns_hi->device || rns_lo->ps != rns_hi->ps) return FHE_ERR_INVALID;
    for (int l = 0; l + 1 < L; ++l)
        if (rns_lo->qs[l] != rns_hi->qs[l]) return FHE_ERR_INVALID;
    if (!giant || !baby || !present || !diags || !baby_keys || !giant_keys || n_giant < 1 || n_baby < 1) return FHE_ERR_INVALID;
    if (!fhe::hoist_ascending(giant, n_giant) || !fhe::hoist_ascending(baby, n_baby)) return FHE_ERR_INVALID;
    if (size_t(n_giant) * size_t(n_baby) >= fhe::HOIST_MAX_ROWS) return FHE_ERR_UNSUPPORTED;
    const int log_n = ilog2(n);
    for (int j = 0; j < n_baby; ++j) {
        const fhe_ckks_key *k = baby_keys[j];
        if (baby[j] != 0 && (!k || k->rns != rns_hi || k->log_n != log_n)) return FHE_ERR_INVALID;
    }
    for (int i = 0; i < n_giant; ++i) {
        const fhe_ckks_key *k = giant_keys[i];
        if (giant[i] != 0 && (!k || k->rns != rns_lo || k->log_n != log_n)) return FHE_ERR_INVALID;
    }
    std::vector<int> tab(size_t(n_giant) + 1 + size_t(n_giant) * n_baby, 0);
    int max_terms = 0;
    const int terms = fhe::hoist_terms(present, n_giant, n_baby, tab.data(), &max_terms);
    if (terms == 0) return FHE_ERR_INVALID;
    tab.resize(size_t(n_giant) + 1 + terms);
    if (size_t(terms) * lk >= fhe::HOIST_MAX_ROWS || (n >> 30)) return FHE_ERR_UNSUPPORTED;
    DeviceGuard guard(rns_hi->device);
    if (!guard.ok) return FHE_ERR_HIP;
    fhe_ckks_diag_matrix_hoisted *m = new (std::nothrow) fhe_ckks_diag_matrix_hoisted();
    if (!m) return FHE_ERR_INVALID;
    m->hi = rns_hi; m->lo = rns_lo; m->device = rns_hi->device; m->log_n = log_n; m->n_giant = n_giant; m->n_baby = n_baby; m->terms = terms; m->max_terms = max_terms;
    // the tables the kernel reads: key pointers and floor(2^64 / modulus), then the 4-byte ones
    std::vector<uint64_t> w8(size_t(2) * n_baby + lk, 0);
    std::vector<unsigned> t_baby(n_baby, 0);
    int bits = 0;
    for (int j = 0; j < n_baby; ++j) {
        const unsigned t = baby[j] ? pow5(baby[j], n) : 0;
        t_baby[j] = t;
        if (t_baby[j]) {
            w8[j] = (uint64_t)(uintptr_t)baby_keys[j]->d_kb;
            w8[size_t(n_baby) + j] = (uint64_t)(uintptr_t)baby_keys[j]->d_ka;
        }
    }
    for (int l = 0; l < lk; ++l) {
        const uint64_t q = l < L ? rns_hi->qs[l] : rns_hi->ps[l - L];
        w8[size_t(2) * n_baby + l] = (uint64_t)(((unsigned __int128)1 << 64) / q);
        if (fhe::hoist_bits(q) > bits) bits = fhe::hoist_bits(q);
    }
    m->fold = fhe::hoist_fold_bound(bits);
    for (int i = 0; i < n_giant; ++i) m->t_giant.push_back(giant[i] ? pow5(giant[i], n) : 0);
    m->baby_keys.assign(baby_keys, baby_keys + n_baby);
    m->giant_keys.assign(giant_keys, giant_keys + n_giant);
    const size_t b8 = w8.size() * sizeof(uint64_t), b_terms = tab.size() * sizeof(int), b_t = t_baby.size() * sizeof(unsigned);
    const size_t words = size_t(terms) * lk * n;
    hipError_t e = hipMalloc((void **)&m->d_diag, words * sizeof(u64));
    if (e == hipSuccess) e = hipMalloc(&m->d_tab, b8 + b_terms + b_t);
    unsigned char *tb = (unsigned char *)m->d_tab;
    if (e == hipSuccess) e = hipMemcpy(tb, w8.data(), b8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tb + b8, tab.data(), b_terms, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tb + b8 + b_terms, t_baby.data(), b_t, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->d_diag, diags, words * sizeof(u64), mem == FHE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) { g_last_hip = (int)e; rc = FHE_ERR_HIP; }
    if (rc == FHE_OK) {
        m->d_kb = (const u64 *const *)tb;
        m->d_ka = m->d_kb + n_baby;
        m->d_mu = (const u64 *)(m->d_ka + n_baby);
        m->d_terms = (const int *)(tb + b8);
        m->d_t = (const unsigned *)(tb + b8 + b_terms);
        // the diagonals: transformed once over qs || ps
        rc = fhe::ntt_fwd_multi(rns_hi->d_descs, (unsigned)lk, m->d_diag, log_n, size_t(terms) * lk, nullptr, rns_hi->all_pm);
    }
    if (hipDeviceSynchronize() != hipSuccess && rc == FHE_OK) rc = FHE_ERR_HIP;
    if (rc != FHE_OK) { fhe_ckks_diag_matrix_hoisted_destroy(m); return rc; }
    *out = m;
    return FHE_OK;
}

int fhe_ckks_mul_mat_hoisted(const fhe_ckks_diag_matrix_hoisted *m, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b, uint64_t *out_a,
                             size_t batch, fhe_mem mem, void *stream) {
    if (!m || ((!ct_b || !ct_a || !out_b || !out_a) && batch)) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    const fhe_rns_ctx *hi = m->hi, *lo = m->lo;
    const int log_n = m->log_n;
    const size_t n = size_t(1) << log_n, L = hi->L, K = hi->K, lk = L + K, Ll = L - 1, ng = m->n_giant;
    fhe::HoistMatWs lay;
    if (!fhe::hoist_mat_ws(n, L, K, batch, ng, &lay)) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(hi->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t in_w = batch * L * n, out_w = batch * Ll * n;
    Mirror mb(ct_b, in_w, mem, true, st), ma(ct_a, in_w, mem, true, st), mob(out_b, out_w, mem, false, st), moa(out_a, out_w, mem, false, st);
    if (mb.rc | ma.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    StreamWs wsp(lay.total * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ws = wsp.as<u64>(), *ext = ws + lay.ext, *bh = ws + lay.bh, *w = ws + lay.w, *x = ws + lay.x, *tmp = ws + lay.tmp, *acc = w;
    const fhe::Barrett *bar_hi = hi->d_barrett, *bar_lo = lo->d_barrett;
    // (a) the lift: one extension, 2 L + K forward transforms
    FHE_TRY(hoist_lift(hi, mb.d, ma.d, ext, bh, log_n, batch, st));
    // (b) every giant step's sum over qs || ps, the baby-step key switches inside it
    const fhe::MatTerms terms{m->d_terms, m->d_terms + ng + 1};
    const fhe::HoistBabies babies{m->d_kb, m->d_ka, m->d_t};
    const size_t rows = ng * 2 * batch * lk;
    FHE_TRY(fhe::with_bool(m->max_terms > m->fold, [&](auto FOLD) {
        return fhe::launch<fhe::ckks_hoist_mac_kernel<FOLD()>>(pair_grid(n, rows), 256, 0, st, (const u64 *)ext, (const u64 *)bh, (const u64 *)m->d_diag, w, terms,
                                                               babies, log_n, (unsigned)L, (unsigned)lk, batch, rows, m->fold, hi->resc.half_q, bar_hi, m->d_mu);
    }));
    // (c) back to coefficients, the division by P, the rescale: 2 (L + K) inverse transforms per giant step
    FHE_TRY(fhe::ntt_inv_multi(hi->d_descs, (unsigned)lk, w, log_n, rows, st, hi->all_pm));
    FHE_TRY(fhe::ckks_rescale_k_dev(hi, w, x, n, ng * 2 * batch, st));
    FHE_TRY(fhe::ckks_rescale_last_dev(hi, x, acc, n, ng * 2 * batch, st));  // w is dead: acc takes its place
    // (d) giant steps on rns_lo, then their sum: fhe_ckks_mul_mat's (f)
    for (size_t i = 0; i < ng; ++i) {
        if (m->t_giant[i] == 0) continue;
        u64 *sb = acc + i * 2 * out_w, *sa = sb + out_w;
        const dim3 g = coeff_grid(n, batch * Ll);
        FHE_TRY(fhe::launch<fhe::rns_automorphism_kernel>(g, 256, 0, st, (const u64 *)sb, tmp, (unsigned)n, (unsigned)Ll, batch * Ll, m->t_giant[i], bar_lo));
        FHE_TRY(fhe::launch<fhe::rns_automorphism_kernel>(g, 256, 0, st, (const u64 *)sa, tmp + out_w, (unsigned)n, (unsigned)Ll, batch * Ll, m->t_giant[i], bar_lo));
        FHE_TRY(fhe::ckks_key_switch_dev(lo, m->giant_keys[i], tmp + out_w, tmp, nullptr, sb, sa, batch, st));
    }
    const dim3 gs = pair_grid(n, batch * Ll);
    FHE_TRY(fhe::launch<fhe::ckks_mat_sum_kernel>(gs, 256, 0, st, (const u64 *)acc, 2 * out_w, (int)ng, mob.d, (unsigned)n, (unsigned)Ll, batch * Ll, bar_lo));
    FHE_TRY(fhe::launch<fhe::ckks_mat_sum_kernel>(gs, 256, 0, st, (const u64 *)(acc + out_w), 2 * out_w, (int)ng, moa.d, (unsigned)n, (unsigned)Ll, batch * Ll, bar_lo));
    int rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

}  // extern "C"
