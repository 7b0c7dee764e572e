// extern "C" entry points of the CKKS diagonal-matrix product: scheme/ckks/src/bootstrapping.rs:90-108 `Bootstrapping::mul_mat`
// (index sets: util/src/misc/matrix.rs:45-52, 125-150) as ONE device entry over a matrix prepared once.
//
//     out = sum_i rotate_i( sum_{j in js(i)} mul_constant(diag_rot(i, j), rotate_j(ct)) )                rotate_0 = identity
//
// Composed from fhe_ckks_rotate / fhe_ckks_mul_plain / fhe_rns_add, T terms over L limbs cost about 5 L T transforms: every
// mul_plain transforms its plaintext (L), both halves of the rotated ciphertext (2 L) and inverse-transforms both products (2 L).
// Here every operand is transformed once: the diagonals at prepare time, each baby-step rotation once (2 L each), the sums of
// limbs 0 .. L-2 once per giant step (2 (L - 1) each) and only the last limb once per term (2 each); ckks_matmul_kernels.hpp has
// the identity that makes the sum of the per-term rescales the rescale of the sum, bit for bit.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "api_common.hpp"
#include "ctx.hpp"
#include "dispatch.hpp"
#include "rns_ctx.hpp"
#include "rns_kernels.hpp"
#include "ckks_matmul_kernels.hpp"

struct fhe_ckks_diag_matrix {
    const fhe_rns_ctx *hi = nullptr, *lo = nullptr;
    int device = -1;                       // hi->device, kept so that destroy does not read the (borrowed) context
    int log_n = 0, n_giant = 0, n_baby = 0, terms = 0;
    int max_terms = 0;                     // the longest giant step (J of the multiply-accumulate)
    int fold = 0;                          // mat_fold_bound of the widest of limbs 0 .. L-2
    std::vector<unsigned> t_baby, t_giant; // 5^j mod 2n, 5^i mod 2n (0 where the index is 0: no rotation)
    std::vector<const fhe_ckks_key *> baby_keys, giant_keys;  // borrowed
    u64 *d_lo = nullptr, *d_hi = nullptr;  // [terms][L - 1][n] | [terms][n], evaluation domain (one allocation)
    int *d_terms = nullptr;                // term_start [n_giant + 1] | term_baby [terms]
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
// x over pairs of coefficients, y over `rows` polynomials
dim3 pair_grid(size_t n, size_t rows) {
    const size_t gx = (n / 2 + 255) / 256;
    return dim3((unsigned)(gx > 64 ? 64 : gx), (unsigned)(rows > 65535 ? 65535 : rows));
}
// x over the coefficients of one polynomial, one per thread, y over `rows` polynomials (rns_automorphism_kernel)
dim3 coeff_grid(size_t n, size_t rows) {
    const size_t gx = (n + 255) / 256;
    return dim3((unsigned)(gx > 64 ? 64 : gx), (unsigned)(rows > 65535 ? 65535 : rows));
}
bool ascending(const uint32_t *v, int cnt) {
    for (int i = 1; i < cnt; ++i)
        if (v[i] <= v[i - 1]) return false;
    return true;
}
}  // namespace

extern "C" {

void fhe_ckks_diag_matrix_destroy(fhe_ckks_diag_matrix *m) {
    if (!m) return;
    if (m->device >= 0) {
        DeviceGuard guard(m->device);
        if (m->d_lo) (void)hipFree(m->d_lo);
        if (m->d_terms) (void)hipFree(m->d_terms);
    }
    delete m;
}

int fhe_ckks_diag_matrix_prepare(const fhe_rns_ctx *rns_hi, const fhe_rns_ctx *rns_lo, size_t n, const uint32_t *giant, int n_giant,
                                 const uint32_t *baby, int n_baby, const uint8_t *present, const uint64_t *diags,
                                 const fhe_ckks_key *const *baby_keys, const fhe_ckks_key *const *giant_keys, fhe_mem mem,
                                 fhe_ckks_diag_matrix **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!rns_hi || !rns_lo) return FHE_ERR_INVALID;
    int rc = fhe::ckks_ring_status(rns_hi, n);
    if (rc != FHE_OK) return rc;
    const int L = rns_hi->L;
    if (L < 2) return FHE_ERR_INVALID;  // the rescale of every term would leave no limb
    // rns_lo: the prefix qs[0 .. L-1) with the same ps on the same device
    if (rns_lo->L != L - 1 || rns_lo->K != rns_hi->K || rns_lo->device != rns_hi->device || rns_lo->ps != rns_hi->ps) return FHE_ERR_INVALID;
    for (int l = 0; l + 1 < L; ++l)
        if (rns_lo->qs[l] != rns_hi->qs[l]) return FHE_ERR_INVALID;
    if (!giant || !baby || !present || !diags || !baby_keys || !giant_keys || n_giant < 1 || n_baby < 1) return FHE_ERR_INVALID;
    if (!ascending(giant, n_giant) || !ascending(baby, n_baby)) return FHE_ERR_INVALID;
    const int log_n = ilog2(n);
    for (int j = 0; j < n_baby; ++j) {
        const fhe_ckks_key *k = baby_keys[j];
        if (baby[j] != 0 && (!k || k->rns != rns_hi || k->log_n != log_n)) return FHE_ERR_INVALID;
    }
    for (int i = 0; i < n_giant; ++i) {
        const fhe_ckks_key *k = giant_keys[i];
        if (giant[i] != 0 && (!k || k->rns != rns_lo || k->log_n != log_n)) return FHE_ERR_INVALID;
    }
    std::vector<int> tab(size_t(n_giant) + 1, 0);
    int max_terms = 0;
    for (int i = 0; i < n_giant; ++i) {
        int cnt = 0;
        for (int j = 0; j < n_baby; ++j)
            if (present[size_t(i) * n_baby + j]) { tab.push_back(j); ++cnt; }
        tab[i + 1] = tab[i] + cnt;
        if (cnt > max_terms) max_terms = cnt;
    }
    const int terms = tab[n_giant];
    if (terms == 0) return FHE_ERR_INVALID;
    if (size_t(terms) * L >= (size_t(1) << 30) || (n >> 30)) return FHE_ERR_UNSUPPORTED;
    DeviceGuard guard(rns_hi->device);
    if (!guard.ok) return FHE_ERR_HIP;
    fhe_ckks_diag_matrix *m = new (std::nothrow) fhe_ckks_diag_matrix();
    if (!m) return FHE_ERR_INVALID;
    m->hi = rns_hi; m->lo = rns_lo; m->device = rns_hi->device; m->log_n = log_n; m->n_giant = n_giant; m->n_baby = n_baby; m->terms = terms; m->max_terms = max_terms;
    int bits = 0;
    for (int l = 0; l + 1 < L; ++l) {
        const int b = 64 - __builtin_clzll(rns_hi->qs[l]);
        if (b > bits) bits = b;
    }
    m->fold = fhe::mat_fold_bound(bits);
    for (int j = 0; j < n_baby; ++j) m->t_baby.push_back(baby[j] ? pow5(baby[j], n) : 0);
    for (int i = 0; i < n_giant; ++i) m->t_giant.push_back(giant[i] ? pow5(giant[i], n) : 0);
    m->baby_keys.assign(baby_keys, baby_keys + n_baby);
    m->giant_keys.assign(giant_keys, giant_keys + n_giant);
    // the diagonals: transformed once, limbs 0 .. L-2 and limb L-1 in two blocks
    const size_t words = size_t(terms) * L * n;
    u64 *tmp = nullptr;
    hipError_t e = hipMalloc((void **)&m->d_lo, words * sizeof(u64));
    if (e == hipSuccess) e = hipMalloc((void **)&tmp, words * sizeof(u64));
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_terms, tab.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(m->d_terms, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tmp, diags, words * sizeof(u64), mem == FHE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) { g_last_hip = (int)e; rc = FHE_ERR_HIP; }
    m->d_hi = m->d_lo ? m->d_lo + size_t(terms) * (L - 1) * n : nullptr;
    if (rc == FHE_OK) rc = fhe::ntt_fwd_multi(rns_hi->d_descs, (unsigned)L, tmp, log_n, size_t(terms) * L, nullptr, rns_hi->all_pm);
    if (rc == FHE_OK)
        rc = fhe::launch<fhe::rns_split_limbs_kernel>(grid_for(words), 256, 0, nullptr, (const u64 *)tmp, m->d_lo, m->d_hi, n, (size_t)terms, L, L - 1);
    if (hipDeviceSynchronize() != hipSuccess && rc == FHE_OK) rc = FHE_ERR_HIP;
    if (tmp) (void)hipFree(tmp);
    if (rc != FHE_OK) { fhe_ckks_diag_matrix_destroy(m); return rc; }
    *out = m;
    return FHE_OK;
}

int fhe_ckks_mul_mat(const fhe_ckks_diag_matrix *m, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b, uint64_t *out_a, size_t batch,
                     fhe_mem mem, void *stream) {
    if (!m || ((!ct_b || !ct_a || !out_b || !out_a) && batch)) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    const fhe_rns_ctx *hi = m->hi, *lo = m->lo;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(hi->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const int log_n = m->log_n;
    const size_t n = size_t(1) << log_n, L = hi->L, Ll = L - 1, nb = m->n_baby, ng = m->n_giant, T = m->terms;
    const size_t in_w = batch * L * n, out_w = batch * Ll * n;
    if (nb * 2 * batch * L >= (size_t(1) << 30) || (ng + 1) * 2 * batch * L >= (size_t(1) << 30) || 2 * T * batch >= (size_t(1) << 30)) return FHE_ERR_UNSUPPORTED;
    Mirror mb(ct_b, in_w, mem, true, st), ma(ct_a, in_w, mem, true, st), mob(out_b, out_w, mem, false, st), moa(out_a, out_w, mem, false, st);
    if (mb.rc | ma.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    // rot [n_baby][2][batch][L][n] | acc [n_giant][2][batch][L-1][n] | last [terms][2][batch][n] | tmp [2][batch][L-1][n]
    const size_t rot_w = nb * 2 * in_w, acc_w = ng * 2 * out_w, last_w = T * 2 * batch * n, tmp_w = 2 * out_w;
    StreamWs wsp((rot_w + acc_w + last_w + tmp_w) * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *rot = wsp.as<u64>(), *acc = rot + rot_w, *last = acc + acc_w, *tmp = last + last_w;
    const fhe::Barrett *bar_hi = hi->d_barrett, *bar_lo = lo->d_barrett;
    // (a) baby steps: rotate_j(ct) = key switch of the automorphism (ckks.rs:279-282); j = 0 is the ciphertext itself
    for (size_t j = 0; j < nb; ++j) {
        u64 *rb = rot + j * 2 * in_w, *ra = rb + in_w;
        if (m->t_baby[j] == 0) {
            HIP_TRY(hipMemcpyAsync(rb, mb.d, in_w * sizeof(u64), hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(ra, ma.d, in_w * sizeof(u64), hipMemcpyDeviceToDevice, st));
            continue;
        }
        const dim3 g = coeff_grid(n, batch * L);
        FHE_TRY(fhe::launch<fhe::rns_automorphism_kernel>(g, 256, 0, st, (const u64 *)mb.d, rb, (unsigned)n, (unsigned)L, batch * L, m->t_baby[j], bar_hi));
        FHE_TRY(fhe::launch<fhe::rns_automorphism_kernel>(g, 256, 0, st, (const u64 *)ma.d, ra, (unsigned)n, (unsigned)L, batch * L, m->t_baby[j], bar_hi));
        FHE_TRY(fhe::ckks_key_switch_dev(hi, m->baby_keys[j], ra, rb, nullptr, rb, ra, batch, st));
    }
    // (b) every rotation to the evaluation domain in one launch
    FHE_TRY(fhe::ntt_fwd_multi(hi->d_descs, (unsigned)L, rot, log_n, nb * 2 * batch * L, st, hi->all_pm));
    // (c) the dot products of limbs 0 .. L-2 and the per-term products of limb L-1
    const fhe::MatTerms terms{m->d_terms, m->d_terms + ng + 1};
    FHE_TRY(fhe::with_bool(m->max_terms > m->fold, [&](auto FOLD) {
        return fhe::launch<fhe::ckks_mat_mac_kernel<FOLD()>>(pair_grid(n, ng * 2 * batch * L), 256, 0, st, (const u64 *)rot, (const u64 *)m->d_lo,
                                                             (const u64 *)m->d_hi, acc, last, terms, (unsigned)n, (unsigned)L, batch, ng * 2 * batch * L,
                                                             m->fold, bar_hi, hi->resc.red_mu);
    }));
    // (d) back to coefficients: the sums on rns_lo's moduli, the per-term products on q_{L-1} alone
    FHE_TRY(fhe::ntt_inv_multi(lo->d_descs, (unsigned)Ll, acc, log_n, ng * 2 * batch * Ll, st, lo->all_pm));
    FHE_TRY(fhe::ntt_inv_multi(hi->d_descs + Ll, 1u, last, log_n, T * 2 * batch, st, hi->all_pm));
    // (e) the rescale of each giant step's sum
    FHE_TRY(fhe::launch<fhe::ckks_mat_rescale_kernel>(pair_grid(n, ng * 2 * batch * Ll), 256, 0, st, acc, (const u64 *)last, terms, (unsigned)n, (unsigned)Ll,
                                                      batch, ng * 2 * batch * Ll, hi->resc_last));
    // (f) giant steps on rns_lo, then their sum
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
