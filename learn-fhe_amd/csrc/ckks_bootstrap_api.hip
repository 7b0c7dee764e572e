// extern "C" entry points that close a CKKS bootstrap over the stages the library already has (`coeff_to_slot` / `slot_to_coeff`,
// ckks_linear_api.hip; the `eval_mod` polynomial, ckks_poly_api.hip).  NO REFERENCE LINE: scheme/ckks/src/bootstrapping.rs ends at the
// two linear transforms.  The conventions are the reference's: `Ckks::encode` (scheme/ckks/src/ckks.rs:186-198) puts Re z_i scale in
// coefficient i and Im z_i scale in coefficient n/2 + i, `Ckks::conjugate` (ckks.rs:279-282) is the automorphism X -> X^-1 with the key
// of `Ckks::cjk_gen` (ckks.rs:169-172).
//
//   fhe_ckks_cjk_gen               sk(X^-1) on the device, then fhe_ckks_ksk_gen;
//   fhe_ckks_mod_raise             limb 0 of a ciphertext lifted to centred integers and reduced into every limb of the top context;
//   fhe_ckks_conj_split / _join    R = ct + conj(ct), J = -X^(n/2) (ct - conj(ct)) stacked as one batch, and out = R' + X^(n/2) J';
//   fhe_ckks_eval_mod_plan_create  the scaled-sine recipe as a plan, interpolated on the host;
//   the bootstrapper               the caller's prepared stages and one conjugation key bound together, and ONE call that runs
//                                  mod_raise, coeff_to_slot, conjugate, split, eval_mod on the stacked batch, join, slot_to_coeff.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "api_common.hpp"
#include "ckks_bootstrap_kernels.hpp"
#include "dispatch.hpp"
#include "rns_ctx.hpp"

struct fhe_ckks_bootstrap {
    int device = -1;
    size_t n = 0;
    int d_c2s = 0, d_mod = 0, d_s2c = 0;
    std::vector<const fhe_rns_ctx *> levels;  // borrowed: levels[0 .. d_c2s + d_mod + d_s2c]
    const fhe_ckks_linear_transform *c2s = nullptr, *s2c = nullptr;  // borrowed
    const fhe_ckks_poly_eval *eval = nullptr;                        // borrowed
    fhe_ckks_key *cjk = nullptr;  // owned: the conjugation key cut down to levels[d_c2s]
};

namespace {
inline bool aligned16(std::initializer_list<const void *> ps) {
    uintptr_t acc = 0;
    for (const void *p : ps) acc |= (uintptr_t)p;
    return (acc & 15u) == 0;
}
// the shape checks the three element-wise entries share; FHE_OK with *run = false means "nothing to do"
int glue_status(const fhe_rns_ctx *r, size_t n, size_t batch, bool null_arg, bool *run) {
    *run = false;
    if (!r || (null_arg && batch)) return FHE_ERR_INVALID;
    FHE_TRY(fhe::ckks_ring_status(r, n));
    if (batch == 0) return FHE_OK;
    if (n >> 31 || batch > (size_t(1) << 40) / n) return FHE_ERR_UNSUPPORTED;
    *run = true;
    return FHE_OK;
}

int mod_raise_dev(const fhe_rns_ctx *r, const u64 *in_b, const u64 *in_a, int in_limbs, u64 *out_b, u64 *out_a, size_t n, size_t batch, hipStream_t st) {
    return fhe::with_bool(n >= 4 && aligned16({in_b, in_a, out_b, out_a}), [&](auto WIDE) {
        constexpr int V = WIDE() ? 2 : 1;
        return fhe::launch<fhe::ckks_mod_raise_kernel<V>>(grid_for(2 * batch * (n / V)), 256, 0, st, in_b, in_a, (unsigned)in_limbs, out_b, out_a, (unsigned)n, r->L,
                                                          batch, (const fhe::Barrett *)r->d_barrett, r->resc.red_mu);
    });
}
int conj_split_dev(const fhe_rns_ctx *r, const u64 *ct_b, const u64 *ct_a, const u64 *cj_b, const u64 *cj_a, u64 *out_b, u64 *out_a, size_t n, size_t batch,
                   hipStream_t st) {
    return fhe::with_bool(n >= 4 && aligned16({ct_b, ct_a, cj_b, cj_a, out_b, out_a}), [&](auto WIDE) {
        constexpr int V = WIDE() ? 2 : 1;
        return fhe::launch<fhe::ckks_conj_split_kernel<V>>(grid_for(2 * batch * (n / V)), 256, 0, st, ct_b, ct_a, cj_b, cj_a, out_b, out_a, (unsigned)n, r->L, batch,
                                                           (const fhe::Barrett *)r->d_barrett);
    });
}
int conj_join_dev(const fhe_rns_ctx *r, const u64 *in_b, const u64 *in_a, u64 *out_b, u64 *out_a, size_t n, size_t batch, hipStream_t st) {
    return fhe::with_bool(n >= 4 && aligned16({in_b, in_a, out_b, out_a}), [&](auto WIDE) {
        constexpr int V = WIDE() ? 2 : 1;
        return fhe::launch<fhe::ckks_conj_join_kernel<V>>(grid_for(2 * batch * (n / V)), 256, 0, st, in_b, in_a, out_b, out_a, (unsigned)n, r->L, batch,
                                                          (const fhe::Barrett *)r->d_barrett);
    });
}

// levels[s] over qs[0 .. L - s) with the same ps on the same device (the rule of fhe_ckks_linear_transform_prepare)
bool prefix_chain(const fhe_rns_ctx *const *levels, int count) {
    const fhe_rns_ctx *top = levels[0];
    if (!top || top->L < count) return false;
    for (int s = 1; s < count; ++s) {
        const fhe_rns_ctx *c = levels[s];
        if (!c || c->device != top->device || c->L != top->L - s || c->K != top->K || c->ps != top->ps) return false;
        if (!std::equal(c->qs.begin(), c->qs.end(), top->qs.begin())) return false;
    }
    return true;
}
// a borrowed stage was prepared on exactly levels[from ..]: the same context objects, the same ring degree
bool bound_to(const std::vector<const fhe_rns_ctx *> &have, size_t have_n, const fhe_rns_ctx *const *levels, int from, size_t n) {
    if (have_n != n) return false;
    for (size_t s = 0; s < have.size(); ++s)
        if (have[s] != levels[from + s]) return false;
    return true;
}
}  // namespace

extern "C" {

int fhe_ckks_cjk_gen(const fhe_rns_ctx *r, const uint64_t *sk, size_t n, const fhe_rng *rng, uint64_t stream_id, uint64_t *ksk_b, uint64_t *ksk_a, fhe_mem mem,
                     void *stream) {
    if (!rng || !r || !sk || !ksk_b || !ksk_a) return FHE_ERR_INVALID;
    FHE_TRY(fhe::ckks_ring_status(r, n));
    if (n >> 31) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = size_t(r->L + r->K) * n;
    Mirror msk(sk, n, mem, true, st), mb(ksk_b, words, mem, false, st), ma(ksk_a, words, mem, false, st);
    if (msk.rc | mb.rc | ma.rc) return FHE_ERR_HIP;
    StreamWs ws(n * sizeof(u64), st);
    if (ws.rc != FHE_OK) return ws.rc;
    FHE_TRY(fhe::launch<fhe::ckks_sk_conj_kernel>(grid_for(n), 256, 0, st, (const long long *)msk.d, ws.as<long long>(), (unsigned)n));
    FHE_TRY(fhe_ckks_ksk_gen(r, (const uint64_t *)msk.d, ws.as<uint64_t>(), n, rng, stream_id, (uint64_t *)mb.d, (uint64_t *)ma.d, FHE_MEM_DEVICE, stream));
    int rc = mb.sync_out(st);
    return rc != FHE_OK ? rc : ma.sync_out(st);
}

int fhe_ckks_mod_raise(const fhe_rns_ctx *r, const uint64_t *ct_b, const uint64_t *ct_a, int in_limbs, uint64_t *out_b, uint64_t *out_a, size_t n, size_t batch,
                       fhe_mem mem, void *stream) {
    if (in_limbs < 1 || in_limbs > (1 << 20)) return FHE_ERR_INVALID;
    bool run = false;
    FHE_TRY(glue_status(r, n, batch, !ct_b || !ct_a || !out_b || !out_a, &run));
    if (!run) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t in_w = batch * size_t(in_limbs) * n, out_w = batch * size_t(r->L) * n;
    Mirror mb(ct_b, in_w, mem, true, st), ma(ct_a, in_w, mem, true, st), mob(out_b, out_w, mem, false, st), moa(out_a, out_w, mem, false, st);
    if (mb.rc | ma.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    FHE_TRY(mod_raise_dev(r, mb.d, ma.d, in_limbs, mob.d, moa.d, n, batch, st));
    int rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

int fhe_ckks_conj_split(const fhe_rns_ctx *r, const uint64_t *ct_b, const uint64_t *ct_a, const uint64_t *cj_b, const uint64_t *cj_a, uint64_t *out_b,
                        uint64_t *out_a, size_t n, size_t batch, fhe_mem mem, void *stream) {
    bool run = false;
    FHE_TRY(glue_status(r, n, batch, !ct_b || !ct_a || !cj_b || !cj_a || !out_b || !out_a, &run));
    if (!run) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t w = batch * size_t(r->L) * n;
    Mirror mb(ct_b, w, mem, true, st), ma(ct_a, w, mem, true, st), mcb(cj_b, w, mem, true, st), mca(cj_a, w, mem, true, st), mob(out_b, 2 * w, mem, false, st),
        moa(out_a, 2 * w, mem, false, st);
    if (mb.rc | ma.rc | mcb.rc | mca.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    FHE_TRY(conj_split_dev(r, mb.d, ma.d, mcb.d, mca.d, mob.d, moa.d, n, batch, st));
    int rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

int fhe_ckks_conj_join(const fhe_rns_ctx *r, const uint64_t *in_b, const uint64_t *in_a, uint64_t *out_b, uint64_t *out_a, size_t n, size_t batch, fhe_mem mem,
                       void *stream) {
    bool run = false;
    FHE_TRY(glue_status(r, n, batch, !in_b || !in_a || !out_b || !out_a, &run));
    if (!run) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t w = batch * size_t(r->L) * n;
    Mirror mb(in_b, 2 * w, mem, true, st), ma(in_a, 2 * w, mem, true, st), mob(out_b, w, mem, false, st), moa(out_a, w, mem, false, st);
    if (mb.rc | ma.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    FHE_TRY(conj_join_dev(r, mb.d, ma.d, mob.d, moa.d, n, batch, st));
    int rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

// ---- the eval_mod recipe (host only) --------------------------------------------------------------------------------------------------
int fhe_ckks_eval_mod_plan_create(int K, int r, int degree, double pre, double post, fhe_ckks_poly_plan **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (K < 1 || r < 0 || r > 1024 || degree < 1 || degree > 255 || !std::isfinite(pre) || !std::isfinite(post)) return FHE_ERR_INVALID;
    fhe_ckks_poly_plan *series = nullptr;
    int rc = FHE_OK;
    try {
        // the interpolant at the degree + 1 Chebyshev nodes of the first kind x_k = cos(theta_k), theta_k = pi (2k + 1) / (2 (degree + 1)):
        // c_j = (2 - [j = 0]) / (degree + 1) sum_k f(x_k) cos(j theta_k), summed in long double and rounded once
        const int N = degree + 1;
        const long double pi = 3.14159265358979323846264338327950288L;
        std::vector<long double> theta(N), f(N);
        for (int k = 0; k < N; ++k) {
            theta[k] = pi * (2 * k + 1) / (2.0L * N);
            f[k] = cosl(2.0L * pi * ((long double)K * cosl(theta[k]) - 0.25L) / ldexpl(1.0L, r));
        }
        std::vector<double> coeffs(N);
        for (int j = 0; j < N; ++j) {
            long double acc = 0.0L;
            for (int k = 0; k < N; ++k) acc += f[k] * cosl(j * theta[k]);
            coeffs[j] = (double)(acc * (j ? 2.0L : 1.0L) / N);
        }
        rc = fhe_ckks_poly_plan_create(coeffs.data(), degree, 0, &series);
        int n_series = 0;
        if (rc == FHE_OK) rc = fhe_ckks_poly_plan_info(series, nullptr, &n_series, nullptr);
        std::vector<fhe_ckks_poly_op> ops(size_t(n_series) + 1);
        if (rc == FHE_OK) rc = fhe_ckks_poly_plan_ops(series, ops.data() + 1, n_series);
        if (rc == FHE_OK) {
            auto lin = [](int dst, int mode, int src, double coef, double c0) {
                fhe_ckks_poly_op o{};
                o.kind = FHE_POLY_LIN; o.dst = dst; o.c = -1; o.mode = mode; o.n_terms = 1; o.src[0] = src; o.coef[0] = coef; o.c0 = c0;
                return o;
            };
            auto mul = [](int dst, int a, int alpha) {
                fhe_ckks_poly_op o{};
                o.kind = FHE_POLY_MUL; o.dst = dst; o.a = a; o.b = a; o.alpha = alpha; o.c = -1;
                return o;
            };
            ops[0] = lin(1, 1, 0, pre / K, 0.0);  // u = pre x / K; the series reads register 1, so every register of it moves up by one
            int top = 1;
            for (int s = 1; s <= n_series; ++s) {
                fhe_ckks_poly_op &o = ops[s];
                o.dst += 1;
                if (o.kind == FHE_POLY_MUL) {
                    o.a += 1; o.b += 1;
                    if (o.c >= 0) o.c += 1;
                } else {
                    for (int j = 0; j < o.n_terms; ++j) o.src[j] += 1;
                }
                top = std::max(top, o.dst);
            }
            int y = ops.back().dst, nxt = top + 1;
            for (int s = 0; s < r; ++s) {  // y <- 2 y^2 - 1
                ops.push_back(mul(nxt, y, 2));
                ops.push_back(lin(nxt + 1, 0, nxt, 1.0, -1.0));
                y = nxt + 1; nxt += 2;
            }
            ops.push_back(lin(nxt, 1, y, post / (2.0 * 3.141592653589793), 0.0));
            rc = fhe_ckks_poly_plan_from_ops(ops.data(), (int)ops.size(), out);
        }
    } catch (const std::bad_alloc &) {
        rc = FHE_ERR_INVALID;
    }
    fhe_ckks_poly_plan_destroy(series);
    return rc;
}

// ---- the bootstrapper -------------------------------------------------------------------------------------------------------------------
void fhe_ckks_bootstrap_destroy(fhe_ckks_bootstrap *bs) {
    if (!bs) return;
    fhe_ckks_key_destroy(bs->cjk);
    delete bs;
}

int fhe_ckks_bootstrap_prepare(const fhe_rns_ctx *const *levels, int n_levels, size_t n, const fhe_ckks_linear_transform *c2s, const fhe_ckks_poly_eval *eval,
                               const fhe_ckks_linear_transform *s2c, const uint64_t *cjk_b, const uint64_t *cjk_a, fhe_mem mem, fhe_ckks_bootstrap **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!levels || !c2s || !eval || !s2c || !cjk_b || !cjk_a || n_levels < 1) return FHE_ERR_INVALID;
    size_t n_c2s = 0, n_mod = 0, n_s2c = 0;
    const std::vector<const fhe_rns_ctx *> &lv_c2s = fhe::ckks_linear_transform_levels(c2s, &n_c2s), &lv_mod = fhe::ckks_poly_eval_levels(eval, &n_mod),
                                           &lv_s2c = fhe::ckks_linear_transform_levels(s2c, &n_s2c);
    const int d_c2s = (int)lv_c2s.size() - 1, d_mod = (int)lv_mod.size() - 1, d_s2c = (int)lv_s2c.size() - 1, depth = d_c2s + d_mod + d_s2c;
    if (d_c2s < 0 || d_mod < 0 || d_s2c < 0 || n_levels < depth + 1 || !prefix_chain(levels, depth + 1)) return FHE_ERR_INVALID;
    const fhe_rns_ctx *top = levels[0];
    FHE_TRY(fhe::ckks_ring_status(top, n));
    if (!bound_to(lv_c2s, n_c2s, levels, 0, n) || !bound_to(lv_mod, n_mod, levels, d_c2s, n) || !bound_to(lv_s2c, n_s2c, levels, d_c2s + d_mod, n))
        return FHE_ERR_INVALID;
    DeviceGuard guard(top->device);
    if (!guard.ok) return FHE_ERR_HIP;
    fhe_ckks_bootstrap *bs = new (std::nothrow) fhe_ckks_bootstrap();
    if (!bs) return FHE_ERR_INVALID;
    int rc = FHE_OK;
    uint64_t *key_tmp = nullptr;
    try {
        bs->device = top->device; bs->n = n; bs->d_c2s = d_c2s; bs->d_mod = d_mod; bs->d_s2c = d_s2c;
        bs->c2s = c2s; bs->eval = eval; bs->s2c = s2c;
        bs->levels.assign(levels, levels + depth + 1);
        // the conjugation runs on levels[d_c2s]: rows 0 .. L - d_c2s of the q-limbs and all K p-limbs of the caller's key (the rule of
        // fhe_ckks_linear_transform_prepare)
        const size_t L = (size_t)top->L, K = (size_t)top->K, Ls = L - d_c2s, half = (Ls + K) * n;
        const hipMemcpyKind kind = mem == FHE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        hipError_t err = hipMalloc((void **)&key_tmp, 2 * half * sizeof(u64));
        const uint64_t *src[2] = {cjk_b, cjk_a};
        for (int h = 0; h < 2 && err == hipSuccess; ++h) {
            err = hipMemcpy(key_tmp + h * half, src[h], Ls * n * sizeof(u64), kind);
            if (err == hipSuccess) err = hipMemcpy(key_tmp + h * half + Ls * n, src[h] + L * n, K * n * sizeof(u64), kind);
        }
        if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; }
        if (rc == FHE_OK) rc = fhe_ckks_ksk_prepare(levels[d_c2s], key_tmp, key_tmp + half, n, FHE_MEM_DEVICE, &bs->cjk);
    } catch (const std::bad_alloc &) {
        rc = FHE_ERR_INVALID;
    }
    if (key_tmp) (void)hipFree(key_tmp);
    if (rc != FHE_OK) { fhe_ckks_bootstrap_destroy(bs); return rc; }
    *out = bs;
    return FHE_OK;
}

int fhe_ckks_bootstrap_info(const fhe_ckks_bootstrap *bs, int *depth, int *out_limbs) {
    if (!bs) return FHE_ERR_INVALID;
    const int d = bs->d_c2s + bs->d_mod + bs->d_s2c;
    if (depth) *depth = d;
    if (out_limbs) *out_limbs = bs->levels[0]->L - d;
    return FHE_OK;
}

int fhe_ckks_bootstrap_apply(const fhe_ckks_bootstrap *bs, const uint64_t *ct_b, const uint64_t *ct_a, int in_limbs, uint64_t *out_b, uint64_t *out_a,
                             size_t batch, fhe_mem mem, void *stream) {
    if (!bs || in_limbs < 1 || in_limbs > (1 << 20) || ((!ct_b || !ct_a || !out_b || !out_a) && batch)) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(bs->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t n = bs->n, L = (size_t)bs->levels[0]->L, L1 = L - bs->d_c2s, L2 = L1 - bs->d_mod, L3 = L2 - bs->d_s2c;
    if (batch > (size_t(1) << 35) / (L * n)) return FHE_ERR_UNSUPPORTED;
    const fhe_rns_ctx *top = bs->levels[0], *mid = bs->levels[bs->d_c2s], *low = bs->levels[bs->d_c2s + bs->d_mod];
    Mirror mb(ct_b, batch * in_limbs * n, mem, true, st), ma(ct_a, batch * in_limbs * n, mem, true, st), mob(out_b, batch * L3 * n, mem, false, st),
        moa(out_a, batch * L3 * n, mem, false, st);
    if (mb.rc | ma.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    // workspace, each a (b, a) pair with its own stream-ordered block that is released as soon as its last reader is enqueued: raised
    // [batch][L] | slots, conj [batch][L1] each | stacked [2 batch][L1] | reduced [2 batch][L2] | joined [batch][L2]
    const size_t w0 = batch * L * n, w1 = batch * L1 * n, w2 = batch * L2 * n;
    auto block = [&](size_t words, std::unique_ptr<StreamWs> &ws, uint64_t **p) -> int {
        ws.reset(new StreamWs(words * sizeof(u64), st));
        *p = ws->as<uint64_t>();
        return ws->rc;
    };
    std::unique_ptr<StreamWs> ws_raised, ws_slots, ws_conj, ws_stacked, ws_reduced, ws_joined;
    uint64_t *raised = nullptr, *slots = nullptr, *conj = nullptr, *stacked = nullptr, *reduced = nullptr, *joined = nullptr;
    FHE_TRY(block(2 * w0, ws_raised, &raised));
    FHE_TRY(fhe_ckks_mod_raise(top, (const uint64_t *)mb.d, (const uint64_t *)ma.d, in_limbs, raised, raised + w0, n, batch, FHE_MEM_DEVICE, stream));
    FHE_TRY(block(2 * w1, ws_slots, &slots));
    FHE_TRY(fhe_ckks_linear_transform_apply(bs->c2s, raised, raised + w0, slots, slots + w1, batch, FHE_MEM_DEVICE, stream));
    ws_raised.reset();
    FHE_TRY(block(2 * w1, ws_conj, &conj));
    HIP_TRY(hipMemcpyAsync(conj, slots, 2 * w1 * sizeof(u64), hipMemcpyDeviceToDevice, st));
    FHE_TRY(fhe_ckks_rotate(mid, bs->cjk, -1, conj, conj + w1, batch, FHE_MEM_DEVICE, stream));
    FHE_TRY(block(4 * w1, ws_stacked, &stacked));
    FHE_TRY(fhe_ckks_conj_split(mid, slots, slots + w1, conj, conj + w1, stacked, stacked + 2 * w1, n, batch, FHE_MEM_DEVICE, stream));
    ws_slots.reset();
    ws_conj.reset();
    FHE_TRY(block(4 * w2, ws_reduced, &reduced));
    FHE_TRY(fhe_ckks_poly_apply(bs->eval, stacked, stacked + 2 * w1, reduced, reduced + 2 * w2, 2 * batch, FHE_MEM_DEVICE, stream));
    ws_stacked.reset();
    FHE_TRY(block(2 * w2, ws_joined, &joined));
    FHE_TRY(fhe_ckks_conj_join(low, reduced, reduced + 2 * w2, joined, joined + w2, n, batch, FHE_MEM_DEVICE, stream));
    ws_reduced.reset();
    FHE_TRY(fhe_ckks_linear_transform_apply(bs->s2c, joined, joined + w2, (uint64_t *)mob.d, (uint64_t *)moa.d, batch, FHE_MEM_DEVICE, stream));
    int rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

}  // extern "C"
