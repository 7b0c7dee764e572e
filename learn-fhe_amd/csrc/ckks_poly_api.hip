// extern "C" entry points of the CKKS polynomial evaluation.  No reference line: `Ckks` has no polynomial evaluation (its bootstrapping
// stops before the modular reduction); the pieces follow scheme/ckks/src/ckks.rs:250-263 `Ckks::mul` (tensor, relinearisation, closing
// `rescale()`) and util/src/ring/rns.rs:99-111 `rescale()` (the K == 1 branch, not centred), and constants are scaled the way
// ckks.rs:186-198 `Ckks::encode` scales a slot: multiplied by `scale`, the fraction dropped toward zero.
//
//   fhe_ckks_lincomb   sum_j k_j ct_j + constant in ONE launch, ciphertexts on different levels read by limb prefix;
//   fhe_ckks_mul_eval  `Ckks::mul` on operands that already are in the evaluation domain, with the epilogue alpha out - ct_c;
//   the plan           a host-only baby-step / giant-step (Paterson-Stockmeyer) schedule of those two operations;
//   the evaluator      the plan bound to the caller's per-level contexts: keys cut down per level, every constant reduced per (op, limb) and
//                      uploaded once, and ONE call that keeps every register that feeds a product in the evaluation domain.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <new>
#include <vector>

#include "api_common.hpp"
#include "ckks_poly_kernels.hpp"
#include "dispatch.hpp"
#include "rns_ctx.hpp"

struct fhe_ckks_poly_plan {
    std::vector<fhe_ckks_poly_op> ops;
    std::vector<int> depth;  // per register: rescales between the input and it; -1 = never written
    int max_depth = 0, result = 0;
};

namespace {
typedef unsigned __int128 u128;
constexpr int MAX_REGS = 4096;

// one prepared op: where it runs and its constants in the evaluator's table
struct PolyStep {
    int level = 0;        // levels[level] is the context it runs on
    size_t ktab = 0;      // offset of its [n_terms + 1][limbs] constants (MUL: of the epilogue's, on one limb fewer), in words
    int epi_terms = 0;    // MUL: terms of the epilogue's linear combination (0 = none)
};
}  // namespace

struct fhe_ckks_poly_eval {
    int device = -1;
    size_t n = 0;
    fhe_ckks_poly_plan plan;
    std::vector<const fhe_rns_ctx *> levels;  // borrowed
    std::map<int, fhe_ckks_key *> keys;       // owned: the relinearisation key cut down to each level a MUL runs on
    std::vector<PolyStep> steps;
    std::vector<uint8_t> needs_eval;          // per register: it is an operand of some MUL
    u64 *d_ktab = nullptr;
    int max_mul_limbs = 0;
};

namespace {
// trunc(c * scale) as sign and magnitude, exactly: c = M 2^e with M < 2^53, so M * scale < 2^117 fits 128 bits; the shift by e drops the
// fraction toward zero.  Not finite, or |c * scale| >= 2^126: FHE_ERR_INVALID.
int trunc_scaled(double c, uint64_t scale, bool *neg, u128 *mag) {
    if (!std::isfinite(c)) return FHE_ERR_INVALID;
    *neg = std::signbit(c);
    *mag = 0;
    const double a = std::fabs(c);
    if (a == 0.0) return FHE_OK;
    int e = 0;
    const uint64_t M = (uint64_t)std::ldexp(std::frexp(a, &e), 53);
    e -= 53;
    const u128 prod = (u128)M * scale;
    if (e >= 0) {
        if (prod && (e >= 126 || (prod >> (126 - e)) != 0)) return FHE_ERR_INVALID;
        *mag = prod << (e >= 126 ? 0 : e);
    } else {
        *mag = -e >= 128 ? (u128)0 : prod >> (-e);
        if (*mag >> 126) return FHE_ERR_INVALID;
    }
    return FHE_OK;
}
uint64_t signed_mod(bool neg, u128 mag, uint64_t q) {
    const uint64_t r = (uint64_t)(mag % q);
    return neg && r ? q - r : r;
}
uint64_t i64_mod(int64_t v, uint64_t q) { return signed_mod(v < 0, (u128)(v < 0 ? 0 - (uint64_t)v : (uint64_t)v), q); }

// the [n_terms + 1][ell] constants of one linear combination over qs[0 .. ell): integer mode i_j and k0 = trunc(c0 scale); real mode
// k_j = trunc(c_j scale) and k0 scale (the constant carries scale^2 before the rescale)
int build_ktab(const std::vector<uint64_t> &qs, int ell, bool real, int n_terms, const double *coef, const int64_t *icoef, double c0, uint64_t scale,
               std::vector<uint64_t> &out) {
    out.assign(size_t(n_terms + 1) * ell, 0);
    bool neg = false;
    u128 mag = 0;
    for (int j = 0; j < n_terms; ++j) {
        if (real) FHE_TRY(trunc_scaled(coef[j], scale, &neg, &mag));
        for (int l = 0; l < ell; ++l) out[size_t(j) * ell + l] = real ? signed_mod(neg, mag, qs[l]) : i64_mod(icoef[j], qs[l]);
    }
    FHE_TRY(trunc_scaled(c0, scale, &neg, &mag));
    for (int l = 0; l < ell; ++l) {
        const uint64_t k0 = signed_mod(neg, mag, qs[l]);
        out[size_t(n_terms) * ell + l] = real ? (uint64_t)((u128)k0 * (scale % qs[l]) % qs[l]) : k0;
    }
    return FHE_OK;
}

// the unreduced accumulation needs q < 2^61 on every limb of the launch (ckks_poly_kernels.hpp)
bool wide_ok(const fhe_rns_ctx *r, int ell) {
    for (int l = 0; l < ell; ++l)
        if (r->qs[l] >> 61) return false;
    return true;
}

// the linear combination on device pointers over the first `ell` limbs of r (real: ell == r->L, out on ell - 1 limbs)
int lincomb_dev(const fhe_rns_ctx *r, int ell, bool real, const fhe::PolyTerms &T, const u64 *d_ktab, u64 *out_b, u64 *out_a, size_t n, size_t batch,
                hipStream_t st) {
    const dim3 grid(grid_for(2 * n * batch));
    return fhe::with_bool(real, [&](auto REAL) {
        return fhe::with_bool(wide_ok(r, ell), [&](auto WIDE) {
            return fhe::launch<fhe::ckks_lincomb_kernel<REAL(), WIDE()>>(grid, 256, 0, st, T, d_ktab, (const fhe::Barrett *)r->d_barrett, r->resc_last, out_b,
                                                                         out_a, (unsigned)n, ell, batch);
        });
    });
}

// `Ckks::mul` (ckks.rs:250-263) on evaluation-domain operands x, y [batch][x_limbs / y_limbs][n] read on the L limbs of r, then the
// epilogue out = alpha out - c as an integer linear combination on L - 1 limbs (epi_terms of them, constants at d_epi; 0 = none).
// ws: 5 batch L n words.  out_b, out_a [batch][L - 1][n].
int mul_eval_dev(const fhe_rns_ctx *r, const fhe_ckks_key *rlk, const u64 *xb, const u64 *xa, int x_limbs, const u64 *yb, const u64 *ya, int y_limbs,
                 int epi_terms, const u64 *d_epi, const u64 *cb, const u64 *ca, int c_limbs, u64 *out_b, u64 *out_a, u64 *ws, size_t batch, hipStream_t st) {
    const int log_n = rlk->log_n;
    const size_t n = size_t(1) << log_n, L = r->L, words = batch * L * n;
    u64 *d = ws, *e = ws + 3 * words;
    const size_t gx = (n + 255) / 256, polys = batch * L;
    const dim3 grid((unsigned)(gx > 64 ? 64 : gx), (unsigned)(polys > 65535 ? 65535 : polys));
    FHE_TRY(fhe::launch<fhe::ckks_tensor_prefix_kernel>(grid, 256, 0, st, xb, xa, (unsigned)x_limbs, yb, ya, (unsigned)y_limbs, d, (unsigned)n, (unsigned)L, polys,
                                                        (const fhe::Barrett *)r->d_barrett));
    FHE_TRY(fhe::ntt_inv_multi(r->d_descs, (unsigned)L, d, log_n, 3 * batch * L, st, r->all_pm));
    // (d0, d1) + relinearize(d2) (ckks.rs:262, 265-272), then `rescale()`
    FHE_TRY(fhe::ckks_key_switch_dev(r, rlk, d + 2 * words, d, d + words, e, e + words, batch, st));
    FHE_TRY(fhe::ckks_rescale_last_dev(r, e, out_b, n, batch, st));
    FHE_TRY(fhe::ckks_rescale_last_dev(r, e + words, out_a, n, batch, st));
    if (!epi_terms) return FHE_OK;
    fhe::PolyTerms T{};
    T.n_terms = epi_terms;
    T.b[0] = out_b; T.a[0] = out_a; T.limbs[0] = (unsigned)(L - 1);
    if (epi_terms > 1) { T.b[1] = cb; T.a[1] = ca; T.limbs[1] = (unsigned)c_limbs; }
    return lincomb_dev(r, (int)L - 1, false, T, d_epi, out_b, out_a, n, batch, st);  // in place: term 0 has the output's layout
}

// the epilogue's constants: alpha on term 0, -1 on term 1 (if any), no constant
void epilogue_ktab(const std::vector<uint64_t> &qs, int ell, int alpha, bool with_c, std::vector<uint64_t> &out) {
    const int nt = with_c ? 2 : 1;
    out.assign(size_t(nt + 1) * ell, 0);
    for (int l = 0; l < ell; ++l) {
        out[l] = (uint64_t)alpha % qs[l];
        if (with_c) out[size_t(ell) + l] = qs[l] - 1;
    }
}

// forward transforms of a register's two halves [batch][limbs][n] into eval [2][batch][limbs][n]
int fwd_register(const fhe_rns_ctx *r, const u64 *b, const u64 *a, u64 *eval, int log_n, size_t batch, hipStream_t st) {
    const size_t L = r->L, words = (batch * L) << log_n;
    if (a == b + words) {
        fhe::NttIo io;
        io.src = b; io.src_mod = (unsigned)(2 * batch * L);
        return fhe::ntt_fwd_multi(r->d_descs, (unsigned)L, eval, log_n, 2 * batch * L, st, r->all_pm, io);
    }
    const u64 *src[2] = {b, a};
    for (int h = 0; h < 2; ++h) {
        fhe::NttIo io;
        io.src = src[h]; io.src_mod = (unsigned)(batch * L);
        FHE_TRY(fhe::ntt_fwd_multi(r->d_descs, (unsigned)L, eval + h * words, log_n, batch * L, st, r->all_pm, io));
    }
    return FHE_OK;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
bool is_int_coef(double v) { return std::isfinite(v) && std::fabs(v) <= 9007199254740992.0 && v == std::floor(v); }

// depths, write-before-read and the limits of every op; fills depth / max_depth / result
int finish_plan(fhe_ckks_poly_plan *p) {
    if (p->ops.empty()) return FHE_ERR_INVALID;
    p->depth.assign(1, 0);
    auto readable = [&](int reg) { return reg >= 0 && reg < (int)p->depth.size() && p->depth[reg] >= 0; };
    for (const fhe_ckks_poly_op &o : p->ops) {
        int d = 0;
        if (o.kind == FHE_POLY_MUL) {
            if (!readable(o.a) || !readable(o.b) || (o.alpha != 1 && o.alpha != 2) || (o.c >= 0 && !readable(o.c)) || o.c < -1) return FHE_ERR_INVALID;
            d = std::max(p->depth[o.a], p->depth[o.b]) + 1;
            if (o.c >= 0 && p->depth[o.c] > d) return FHE_ERR_INVALID;  // the subtrahend must have every limb of the product
        } else if (o.kind == FHE_POLY_LIN) {
            if (o.n_terms < 1 || o.n_terms > fhe::POLY_MAX_TERMS || (o.mode != 0 && o.mode != 1) || !std::isfinite(o.c0)) return FHE_ERR_INVALID;
            for (int j = 0; j < o.n_terms; ++j) {
                if (!readable(o.src[j]) || !(o.mode ? std::isfinite(o.coef[j]) : is_int_coef(o.coef[j]))) return FHE_ERR_INVALID;
                d = std::max(d, p->depth[o.src[j]]);
            }
            d += o.mode;
        } else
            return FHE_ERR_INVALID;
        if (o.dst < 1 || o.dst >= MAX_REGS) return FHE_ERR_INVALID;
        if (o.dst >= (int)p->depth.size()) p->depth.resize(size_t(o.dst) + 1, -1);
        if (p->depth[o.dst] >= 0) return FHE_ERR_INVALID;  // every register is written once
        p->depth[o.dst] = d;
    }
    p->result = p->ops.back().dst;
    p->max_depth = 0;
    for (int d : p->depth) p->max_depth = std::max(p->max_depth, d);
    return p->depth[p->result] == p->max_depth ? FHE_OK : FHE_ERR_INVALID;  // the result is the deepest register
}

// the fixed baby-step / giant-step schedule (fhe_ring.h)
struct Builder {
    std::vector<fhe_ckks_poly_op> ops;
    std::map<int, int> power;  // i -> register of T_i (x^i)
    int next = 1, k = 2;
    bool cheb = true;

    int mul(int a, int b, int alpha, int c) {
        fhe_ckks_poly_op o{};
        o.kind = FHE_POLY_MUL; o.dst = next++; o.a = a; o.b = b; o.alpha = alpha; o.c = c;
        ops.push_back(o);
        return o.dst;
    }
    int lin(int mode, const std::vector<std::pair<int, double>> &terms, double c0) {
        fhe_ckks_poly_op o{};
        o.kind = FHE_POLY_LIN; o.dst = next++; o.mode = mode; o.n_terms = (int)terms.size(); o.c0 = c0; o.c = -1;
        for (int j = 0; j < o.n_terms; ++j) { o.src[j] = terms[j].first; o.coef[j] = terms[j].second; }
        ops.push_back(o);
        return o.dst;
    }
    // T_{a+b} = 2 T_a T_b - T_{a-b} with a the largest power of two below i (depth ceil(log2 i)); T_{2a} = 2 T_a^2 - 1; x^{a+b} = x^a x^b
    int pow_reg(int i) {
        if (i == 1) return 0;
        const auto it = power.find(i);
        if (it != power.end()) return it->second;
        int a = 1;
        while (2 * a < i) a *= 2;
        const int b = i - a;
        int reg;
        if (!cheb) {
            const int ra = pow_reg(a), rb = pow_reg(b);
            reg = mul(ra, rb, 1, -1);
        } else if (a == b) {
            const int h = pow_reg(a);
            reg = lin(0, {{mul(h, h, 2, -1), 1.0}}, -1.0);
        } else {
            const int ra = pow_reg(a), rb = pow_reg(b), rc = pow_reg(a - b);
            reg = mul(ra, rb, 2, rc);
        }
        power[i] = reg;
        return reg;
    }
    // the register of sum_j c_j T_j, or -1 where every c_j is zero
    int eval(std::vector<double> c) {
        while (!c.empty() && c.back() == 0.0) c.pop_back();
        if (c.empty()) return -1;
        const int d = (int)c.size() - 1;
        if (d < k) {  // a block: one real-mode combination of the baby powers
            std::vector<std::pair<int, double>> terms;
            for (int j = 1; j <= d; ++j)
                if (c[j] != 0.0) terms.push_back({pow_reg(j), c[j]});
            if (terms.empty()) terms.push_back({0, 0.0});
            return lin(1, terms, c[0]);
        }
        int m = k;
        while (2 * m <= d) m *= 2;
        // p = quo T_m + rem: T_{m+i} = 2 T_m T_i - T_{m-i}, x^{m+i} = x^m x^i
        std::vector<double> quo(size_t(d - m) + 1), rem(m);
        for (int i = 0; i <= d - m; ++i) quo[i] = cheb && i ? 2.0 * c[m + i] : c[m + i];
        for (int j = 0; j < m; ++j) {
            rem[j] = c[j];
            if (cheb && j && 2 * m - j <= d) rem[j] -= c[2 * m - j];
            rem[j] = -rem[j];  // the product's epilogue subtracts: quo T_m - (-rem)
        }
        const int rq = eval(quo), rr = eval(rem), g = pow_reg(m);
        return mul(rq, g, 1, rr);
    }
};
}  // namespace

extern "C" {

int fhe_ckks_scaled_constant(double c, uint64_t scale, uint64_t q, uint64_t *out) {
    if (!out || scale == 0 || q < 2) return FHE_ERR_INVALID;
    bool neg = false;
    u128 mag = 0;
    FHE_TRY(trunc_scaled(c, scale, &neg, &mag));
    *out = signed_mod(neg, mag, q);
    return FHE_OK;
}

int fhe_ckks_lincomb(const fhe_rns_ctx *r, int real, int n_terms, const uint64_t *const *ct_b, const uint64_t *const *ct_a, const int *limbs,
                     const int64_t *imul, const double *cmul, double c0, uint64_t scale, uint64_t *out_b, uint64_t *out_a, size_t n, size_t batch,
                     fhe_mem mem, void *stream) {
    if (!r || !ct_b || !ct_a || !limbs || n_terms < 1 || n_terms > fhe::POLY_MAX_TERMS || scale == 0 || (real ? !cmul : !imul)) return FHE_ERR_INVALID;
    FHE_TRY(fhe::ckks_ring_status(r, n));
    const int ell = r->L;
    if (real && ell < 2) return FHE_ERR_INVALID;
    for (int j = 0; j < n_terms; ++j)
        if (limbs[j] < ell || limbs[j] > (1 << 20) || ((!ct_b[j] || !ct_a[j]) && batch)) return FHE_ERR_INVALID;
    if ((!out_b || !out_a) && batch) return FHE_ERR_INVALID;
    std::vector<uint64_t> ktab;
    FHE_TRY(build_ktab(r->qs, ell, real != 0, n_terms, cmul, imul, c0, scale, ktab));
    if (batch == 0) return FHE_OK;
    if (n >> 31 || batch > (size_t(1) << 40) / n) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    std::vector<std::unique_ptr<Mirror>> ins;
    fhe::PolyTerms T{};
    T.n_terms = n_terms;
    for (int j = 0; j < n_terms; ++j) {
        const size_t w = batch * size_t(limbs[j]) * n;
        ins.emplace_back(new Mirror(ct_b[j], w, mem, true, st));
        ins.emplace_back(new Mirror(ct_a[j], w, mem, true, st));
        if (ins[2 * j]->rc | ins[2 * j + 1]->rc) return FHE_ERR_HIP;
        T.b[j] = ins[2 * j]->d; T.a[j] = ins[2 * j + 1]->d; T.limbs[j] = (unsigned)limbs[j];
    }
    const size_t out_w = batch * size_t(real ? ell - 1 : ell) * n;
    Mirror mob(out_b, out_w, mem, false, st), moa(out_a, out_w, mem, false, st);
    if (mob.rc | moa.rc) return FHE_ERR_HIP;
    StreamWs ws(ktab.size() * sizeof(u64), st);
    if (ws.rc != FHE_OK) return ws.rc;
    HIP_TRY(hipMemcpyAsync(ws.p, ktab.data(), ktab.size() * sizeof(u64), hipMemcpyHostToDevice, st));
    int rc = lincomb_dev(r, ell, real != 0, T, ws.as<u64>(), mob.d, moa.d, n, batch, st);
    if (hipStreamSynchronize(st) != hipSuccess && rc == FHE_OK) rc = FHE_ERR_HIP;  // ktab is a stack-owned vector
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

int fhe_ckks_mul_eval(const fhe_rns_ctx *r, const fhe_ckks_key *rlk, const uint64_t *x_b, const uint64_t *x_a, int x_limbs, const uint64_t *y_b,
                      const uint64_t *y_a, int y_limbs, int alpha, const uint64_t *c_b, const uint64_t *c_a, int c_limbs, uint64_t *out_b, uint64_t *out_a,
                      size_t batch, fhe_mem mem, void *stream) {
    if (!r || !rlk || rlk->rns != r || (alpha != 1 && alpha != 2) || (!c_b != !c_a)) return FHE_ERR_INVALID;
    if (((!x_b || !x_a || !y_b || !y_a || !out_b || !out_a) && batch) || r->L < 2) return FHE_ERR_INVALID;
    if (r->device < 0) return FHE_ERR_NO_DEVICE;
    const int L = r->L;
    if (x_limbs < L || y_limbs < L || x_limbs > (1 << 20) || y_limbs > (1 << 20) || (c_b && (c_limbs < L - 1 || c_limbs > (1 << 20)))) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    const size_t n = size_t(1) << rlk->log_n;
    if (n < 2 || n >> 31 || batch > (size_t(1) << 40) / n) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t xw = batch * x_limbs * n, yw = batch * y_limbs * n, cw = c_b ? batch * c_limbs * n : 0, ow = batch * size_t(L - 1) * n;
    Mirror mxb(x_b, xw, mem, true, st), mxa(x_a, xw, mem, true, st), myb(y_b, yw, mem, true, st), mya(y_a, yw, mem, true, st), mcb(c_b, cw, mem, true, st),
        mca(c_a, cw, mem, true, st), mob(out_b, ow, mem, false, st), moa(out_a, ow, mem, false, st);
    if (mxb.rc | mxa.rc | myb.rc | mya.rc | mcb.rc | mca.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    const int epi_terms = c_b ? 2 : (alpha == 2 ? 1 : 0);
    std::vector<uint64_t> ktab;
    epilogue_ktab(r->qs, L - 1, alpha, c_b != nullptr, ktab);
    StreamWs ws((5 * batch * L * n + ktab.size()) * sizeof(u64), st);
    if (ws.rc != FHE_OK) return ws.rc;
    u64 *d_epi = ws.as<u64>() + 5 * batch * L * n;
    HIP_TRY(hipMemcpyAsync(d_epi, ktab.data(), ktab.size() * sizeof(u64), hipMemcpyHostToDevice, st));
    int rc = mul_eval_dev(r, rlk, mxb.d, mxa.d, x_limbs, myb.d, mya.d, y_limbs, epi_terms, d_epi, mcb.d, mca.d, c_limbs, mob.d, moa.d, ws.as<u64>(), batch, st);
    if (hipStreamSynchronize(st) != hipSuccess && rc == FHE_OK) rc = FHE_ERR_HIP;  // ktab is a stack-owned vector
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

// ---- the plan (host only) ------------------------------------------------------------------------------------------------------------
void fhe_ckks_poly_plan_destroy(fhe_ckks_poly_plan *p) { delete p; }

int fhe_ckks_poly_plan_create(const double *coeffs, int degree, int basis, fhe_ckks_poly_plan **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!coeffs || degree < 0 || degree > 255 || (basis != 0 && basis != 1)) return FHE_ERR_INVALID;
    for (int j = 0; j <= degree; ++j)
        if (!std::isfinite(coeffs[j])) return FHE_ERR_INVALID;
    fhe_ckks_poly_plan *p = nullptr;
    try {
        Builder bld;
        bld.cheb = basis == 0;
        while (bld.k * bld.k < degree + 1) bld.k *= 2;
        if (bld.eval(std::vector<double>(coeffs, coeffs + degree + 1)) < 0) bld.lin(1, {{0, 0.0}}, 0.0);  // the zero polynomial
        p = new fhe_ckks_poly_plan();
        p->ops = std::move(bld.ops);
    } catch (const std::bad_alloc &) {
        delete p;
        return FHE_ERR_INVALID;
    }
    const int rc = finish_plan(p);
    if (rc != FHE_OK) { delete p; return rc; }
    *out = p;
    return FHE_OK;
}

int fhe_ckks_poly_plan_from_ops(const fhe_ckks_poly_op *ops, int n_ops, fhe_ckks_poly_plan **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!ops || n_ops < 1 || n_ops > MAX_REGS) return FHE_ERR_INVALID;
    fhe_ckks_poly_plan *p = new (std::nothrow) fhe_ckks_poly_plan();
    if (!p) return FHE_ERR_INVALID;
    int rc = FHE_OK;
    try {
        p->ops.assign(ops, ops + n_ops);
        rc = finish_plan(p);
    } catch (const std::bad_alloc &) { rc = FHE_ERR_INVALID; }
    if (rc != FHE_OK) { delete p; return rc; }
    *out = p;
    return FHE_OK;
}

int fhe_ckks_poly_plan_info(const fhe_ckks_poly_plan *p, int *depth, int *n_ops, int *n_regs) {
    if (!p) return FHE_ERR_INVALID;
    if (depth) *depth = p->max_depth;
    if (n_ops) *n_ops = (int)p->ops.size();
    if (n_regs) *n_regs = (int)p->depth.size();
    return FHE_OK;
}

int fhe_ckks_poly_plan_ops(const fhe_ckks_poly_plan *p, fhe_ckks_poly_op *out, int count) {
    if (!p || (!out && count) || count < 0 || count > (int)p->ops.size()) return FHE_ERR_INVALID;
    std::copy(p->ops.begin(), p->ops.begin() + count, out);
    return FHE_OK;
}

// ---- the prepared evaluator ---------------------------------------------------------------------------------------------------------
void fhe_ckks_poly_eval_destroy(fhe_ckks_poly_eval *ev) {
    if (!ev) return;
    for (auto &k : ev->keys) fhe_ckks_key_destroy(k.second);
    if (ev->d_ktab && ev->device >= 0) {
        DeviceGuard guard(ev->device);
        (void)hipFree(ev->d_ktab);
    }
    delete ev;
}

int fhe_ckks_poly_prepare(const fhe_ckks_poly_plan *p, const fhe_rns_ctx *const *levels, int n_levels, uint64_t scale, const uint64_t *rlk_b,
                          const uint64_t *rlk_a, size_t n, fhe_mem mem, fhe_ckks_poly_eval **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!p || !levels || !rlk_b || !rlk_a || scale == 0) return FHE_ERR_INVALID;
    const int depth = p->max_depth;
    if (n_levels < depth + 1) return FHE_ERR_INVALID;
    const fhe_rns_ctx *top = levels[0];
    if (!top || top->L < depth + 1) return FHE_ERR_INVALID;
    FHE_TRY(fhe::ckks_ring_status(top, n));
    if (n < 2) return FHE_ERR_INVALID;
    const int L = top->L, K = top->K;
    for (int s = 1; s <= depth; ++s) {  // levels[s]: qs[0 .. L - s) with the same ps on the same device
        const fhe_rns_ctx *c = levels[s];
        if (!c || c->device != top->device || c->L != L - s || c->K != K || c->ps != top->ps) return FHE_ERR_INVALID;
        if (!std::equal(c->qs.begin(), c->qs.end(), top->qs.begin())) return FHE_ERR_INVALID;
    }
    DeviceGuard guard(top->device);
    if (!guard.ok) return FHE_ERR_HIP;
    fhe_ckks_poly_eval *ev = new (std::nothrow) fhe_ckks_poly_eval();
    if (!ev) return FHE_ERR_INVALID;
    int rc = FHE_OK;
    uint64_t *key_tmp = nullptr;
    try {
        ev->device = top->device; ev->n = n; ev->plan = *p;
        ev->levels.assign(levels, levels + depth + 1);
        ev->needs_eval.assign(p->depth.size(), 0);
        std::vector<uint64_t> table, one;
        for (const fhe_ckks_poly_op &o : p->ops) {
            PolyStep s;
            s.ktab = table.size();
            if (o.kind == FHE_POLY_MUL) {
                s.level = std::max(p->depth[o.a], p->depth[o.b]);
                ev->needs_eval[o.a] = ev->needs_eval[o.b] = 1;
                ev->max_mul_limbs = std::max(ev->max_mul_limbs, L - s.level);
                s.epi_terms = o.c >= 0 ? 2 : (o.alpha == 2 ? 1 : 0);
                epilogue_ktab(top->qs, L - s.level - 1, o.alpha, o.c >= 0, one);
                ev->keys[s.level] = nullptr;
            } else {
                for (int j = 0; j < o.n_terms; ++j) s.level = std::max(s.level, p->depth[o.src[j]]);
                int64_t ic[fhe::POLY_MAX_TERMS] = {};
                if (!o.mode)
                    for (int j = 0; j < o.n_terms; ++j) ic[j] = (int64_t)o.coef[j];
                rc = build_ktab(top->qs, L - s.level, o.mode != 0, o.n_terms, o.coef, ic, o.c0, scale, one);
                if (rc != FHE_OK) break;
            }
            table.insert(table.end(), one.begin(), one.end());
            ev->steps.push_back(s);
        }
        hipError_t err = hipSuccess;
        if (rc == FHE_OK) {
            err = hipMalloc((void **)&ev->d_ktab, table.size() * sizeof(u64));
            if (err == hipSuccess) err = hipMemcpy(ev->d_ktab, table.data(), table.size() * sizeof(u64), hipMemcpyHostToDevice);
            if (err == hipSuccess && !ev->keys.empty()) err = hipMalloc((void **)&key_tmp, 2 * size_t(L + K) * n * sizeof(uint64_t));
            if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; }
        }
        // the key on levels[s]: rows 0 .. L - s of the q-limbs and all K p-limbs of the caller's key (the reference's key switch at a lower
        // level multiplies on the limbs both sides have, rns.rs:148-158)
        const hipMemcpyKind kind = mem == FHE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        for (auto &k : ev->keys) {
            if (rc != FHE_OK) break;
            const size_t Ls = size_t(L - k.first), half = (Ls + K) * n;
            const uint64_t *src[2] = {rlk_b, rlk_a};
            for (int h = 0; h < 2 && err == hipSuccess; ++h) {
                err = hipMemcpy(key_tmp + h * half, src[h], Ls * n * sizeof(u64), kind);
                if (err == hipSuccess) err = hipMemcpy(key_tmp + h * half + Ls * n, src[h] + size_t(L) * n, size_t(K) * n * sizeof(u64), kind);
            }
            if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; break; }
            rc = fhe_ckks_ksk_prepare(levels[k.first], key_tmp, key_tmp + half, n, FHE_MEM_DEVICE, &k.second);
        }
    } catch (const std::bad_alloc &) {
        rc = FHE_ERR_INVALID;
    }
    if (key_tmp) (void)hipFree(key_tmp);
    if (rc != FHE_OK) { fhe_ckks_poly_eval_destroy(ev); return rc; }
    *out = ev;
    return FHE_OK;
}

int fhe_ckks_poly_apply(const fhe_ckks_poly_eval *ev, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b, uint64_t *out_a, size_t batch, fhe_mem mem,
                        void *stream) {
    if (!ev || ((!ct_b || !ct_a || !out_b || !out_a) && batch)) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(ev->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const fhe_ckks_poly_plan &P = ev->plan;
    const size_t n = ev->n, L = (size_t)ev->levels[0]->L;
    const int log_n = ilog2(n);
    if (batch > (size_t(1) << 36) / (L * n)) return FHE_ERR_UNSUPPORTED;
    const size_t in_w = batch * L * n, out_w = batch * (L - P.max_depth) * n;
    Mirror mb(ct_b, in_w, mem, true, st), ma(ct_a, in_w, mem, true, st), mob(out_b, out_w, mem, false, st), moa(out_a, out_w, mem, false, st);
    if (mb.rc | ma.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    // workspace: every register but the input and the result in the coefficient domain, the operands of products in the evaluation
    // domain as well, and one product's scratch
    const int n_regs = (int)P.depth.size();
    std::vector<size_t> coef_off(n_regs, 0), eval_off(n_regs, 0);
    size_t total = 5 * batch * size_t(ev->max_mul_limbs) * n;
    for (int g = 0; g < n_regs; ++g) {
        if (P.depth[g] < 0) continue;
        const size_t w = 2 * batch * (L - P.depth[g]) * n;
        if (g != 0 && g != P.result) { coef_off[g] = total; total += w; }
        if (ev->needs_eval[g]) { eval_off[g] = total; total += w; }
    }
    StreamWs ws(total * sizeof(u64), st);
    if (ws.rc != FHE_OK) return ws.rc;
    u64 *base = ws.as<u64>();
    auto reg_b = [&](int g) -> u64 * { return g == 0 ? mb.d : g == P.result ? mob.d : base + coef_off[g]; };
    auto reg_a = [&](int g) -> u64 * { return g == 0 ? ma.d : g == P.result ? moa.d : base + coef_off[g] + batch * (L - P.depth[g]) * n; };
    auto to_eval = [&](int g) -> int {
        return ev->needs_eval[g] ? fwd_register(ev->levels[P.depth[g]], reg_b(g), reg_a(g), base + eval_off[g], log_n, batch, st) : FHE_OK;
    };
    FHE_TRY(to_eval(0));
    for (size_t s = 0; s < P.ops.size(); ++s) {
        const fhe_ckks_poly_op &o = P.ops[s];
        const PolyStep &S = ev->steps[s];
        const fhe_rns_ctx *r = ev->levels[S.level];
        if (o.kind == FHE_POLY_MUL) {
            const size_t ha = batch * (L - P.depth[o.a]) * n, hb = batch * (L - P.depth[o.b]) * n;
            const u64 *xa = base + eval_off[o.a], *xb = base + eval_off[o.b];
            FHE_TRY(mul_eval_dev(r, ev->keys.at(S.level), xa, xa + ha, (int)(L - P.depth[o.a]), xb, xb + hb, (int)(L - P.depth[o.b]), S.epi_terms,
                                 ev->d_ktab + S.ktab, o.c >= 0 ? reg_b(o.c) : nullptr, o.c >= 0 ? reg_a(o.c) : nullptr, o.c >= 0 ? (int)(L - P.depth[o.c]) : 0,
                                 reg_b(o.dst), reg_a(o.dst), base, batch, st));
        } else {
            fhe::PolyTerms T{};
            T.n_terms = o.n_terms;
            for (int j = 0; j < o.n_terms; ++j) { T.b[j] = reg_b(o.src[j]); T.a[j] = reg_a(o.src[j]); T.limbs[j] = (unsigned)(L - P.depth[o.src[j]]); }
            FHE_TRY(lincomb_dev(r, r->L, o.mode != 0, T, ev->d_ktab + S.ktab, reg_b(o.dst), reg_a(o.dst), n, batch, st));
        }
        FHE_TRY(to_eval(o.dst));
    }
    int rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

}  // extern "C"

namespace fhe {
const std::vector<const fhe_rns_ctx *> &ckks_poly_eval_levels(const fhe_ckks_poly_eval *ev, size_t *n) {
    *n = ev->n;
    return ev->levels;
}
}  // namespace fhe
