// extern "C" entry points of the CKKS linear transforms `coeff_to_slot` / `slot_to_coeff`: scheme/ckks/src/bootstrapping.rs:23-31
// `BootstrappingParam::new` (the plan), bootstrapping.rs:56-71 `key_gen` (the rotation set and fhe_ckks_rtk_gen) and
// bootstrapping.rs:81-88 `mul_mats` (the prepared transform), over scheme/ckks/src/sfft.rs:75-99 and util/src/misc/matrix.rs:45-52,
// 71-83, 94-150.  The matrices are made on the device in the encoder's double-double format from the encoder's own twiddle table;
// the host only does the index arithmetic (which diagonals exist, which pairs feed them, the baby-step / giant-step split).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <new>
#include <utility>
#include <vector>

#include "api_common.hpp"
#include "ckks_encoder.hpp"
#include "ckks_linear_kernels.hpp"
#include "dispatch.hpp"
#include "rns_ctx.hpp"

namespace {
// one matrix of a plan: its diagonal indices (ascending, mod l), their values and `DiagSparseMatrix::bsgs` of the indices
struct LinMat {
    std::vector<uint32_t> idx;
    uint32_t k = 1;
    std::vector<uint32_t> giant, baby;
    std::vector<uint8_t> present;  // [giant][baby]
    double4 *d = nullptr;          // [idx.size()][l]; null on a host-only plan
};
}  // namespace

struct fhe_ckks_linear_plan {
    const fhe_ckks_encoder *enc = nullptr;  // borrowed
    unsigned l = 0;
    int log_l = 0, r = 0, inverse = 0, device = -1;
    std::vector<LinMat> mats;
    std::vector<uint32_t> rot;  // ascending union of the non-zero giant and baby steps
};

struct fhe_ckks_linear_transform {
    int device = -1;
    size_t n = 0;
    std::vector<const fhe_rns_ctx *> levels;   // borrowed: levels[s] -> levels[s + 1] is step s
    std::vector<fhe_ckks_key *> keys;          // owned: every (level, rotation) key of the steps, restricted to that level
    std::vector<fhe_ckks_diag_matrix *> mats;  // owned, in the order of application
};

namespace {
// matrix.rs:45-52, 125-150 `DiagSparseMatrix::bsgs`: the k in 1..=max index with the fewest distinct non-zero values among all
// i = d - d % k and j = d % k, the smallest such k on a tie (`min_by_key` keeps the first); k = 1 where the only index is 0
void bsgs_split(LinMat &m, unsigned l) {
    const std::vector<uint32_t> &ds = m.idx;
    const uint32_t max_d = ds.back();
    std::vector<uint32_t> stamp(size_t(l) + 1, 0);
    size_t best = ~size_t(0);
    m.k = 1;
    for (uint32_t k = 1; k <= max_d; ++k) {
        size_t cnt = 0;
        for (uint32_t d : ds)
            for (uint32_t v : {d - d % k, d % k})
                if (v && stamp[v] != k) { stamp[v] = k; ++cnt; }
        if (cnt < best) { best = cnt; m.k = k; }
    }
    for (uint32_t d : ds) { m.giant.push_back(d - d % m.k); m.baby.push_back(d % m.k); }
    for (std::vector<uint32_t> *v : {&m.giant, &m.baby}) {
        std::sort(v->begin(), v->end());
        v->erase(std::unique(v->begin(), v->end()), v->end());
    }
    m.present.assign(m.giant.size() * m.baby.size(), 0);
    for (uint32_t d : ds) {
        const size_t gi = std::lower_bound(m.giant.begin(), m.giant.end(), d - d % m.k) - m.giant.begin();
        const size_t bj = std::lower_bound(m.baby.begin(), m.baby.end(), d % m.k) - m.baby.begin();
        m.present[gi * m.baby.size() + bj] = 1;
    }
}

// the diagonals of factor log_k (sfft.rs:79-92), of its inverse where inv (matrix.rs:71-83, indices mod l), ascending by index
void factor_diags(unsigned l, unsigned log_k, bool inv, std::vector<uint32_t> &idx, fhe::FactorDiags &D) {
    const unsigned m = l >> (1 + log_k);
    std::vector<std::pair<uint32_t, int>> v;  // (index of the forward factor, which vector)
    v.push_back({0u, 0});
    v.push_back({l - m, 1});
    if (log_k) v.push_back({m, 2});
    std::vector<std::pair<uint32_t, std::pair<int, unsigned>>> o;
    for (const auto &e : v) o.push_back({inv ? (l - e.first) % l : e.first, {e.second, inv ? e.first : 0u}});
    std::sort(o.begin(), o.end());
    idx.clear();
    D.n = (int)o.size();
    for (int s = 0; s < D.n; ++s) { idx.push_back(o[s].first); D.which[s] = o[s].second.first; D.shift[s] = o[s].second.second; }
}

// the index set of a product and, per output diagonal, its pairs in the reference's order (matrix.rs:101-106)
void product_structure(unsigned l, const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, std::vector<uint32_t> &out, std::vector<unsigned> &start,
                       std::vector<fhe::LinPair> &pairs) {
    std::map<uint32_t, std::vector<fhe::LinPair>> groups;
    for (unsigned i = 0; i < a.size(); ++i)
        for (unsigned j = 0; j < b.size(); ++j) groups[(a[i] + b[j]) % l].push_back(fhe::LinPair{i, j, a[i]});
    out.clear(); start.assign(1, 0u); pairs.clear();
    for (const auto &g : groups) {
        out.push_back(g.first);
        pairs.insert(pairs.end(), g.second.begin(), g.second.end());
        start.push_back((unsigned)pairs.size());
    }
}

// A matrix of more than 2^26 elements (2 GiB) is refused: a dense matrix exists only for small l.
constexpr size_t LIN_MAX_ELEMS = size_t(1) << 26;

void free_mats(fhe_ckks_linear_plan *p) {
    for (LinMat &m : p->mats)
        if (m.d) { (void)hipFree(m.d); m.d = nullptr; }
}

// the values of every matrix: one launch per factor, one per product; runs on the null stream and waits for it
int fill_values(fhe_ckks_linear_plan *p) {
    const fhe_ckks_encoder *e = p->enc;
    const unsigned l = p->l;
    const int log_l = p->log_l, depth = (int)p->mats.size();
    const fhe::EncTables T{e->d_tw, e->d_pow5, (unsigned)log_l};
    int rc = FHE_OK;
    std::vector<uint32_t> f_idx, acc_idx, out_idx;
    std::vector<unsigned> start;
    std::vector<fhe::LinPair> pairs;
    for (int c = 0; c < depth && rc == FHE_OK; ++c) {
        double4 *acc = nullptr;
        const int lo = c * p->r, hi = std::min(log_l, lo + p->r);
        for (int t = lo; t < hi && rc == FHE_OK; ++t) {
            // sifft_fmats is the reversed list of the inverses (sfft.rs:97-99)
            const unsigned log_k = (unsigned)(p->inverse ? log_l - 1 - t : t);
            fhe::FactorDiags D{};
            factor_diags(l, log_k, p->inverse != 0, f_idx, D);
            double4 *f = nullptr;
            hipError_t err = hipMalloc((void **)&f, (size_t(D.n) << log_l) * sizeof(double4));
            if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; break; }
            rc = fhe::with_bool(p->inverse != 0, [&](auto INV) {
                return fhe::launch<fhe::lin_factor_kernel<INV()>>(grid_for(size_t(D.n) << log_l), 256, 0, nullptr, T, log_k, D, f);
            });
            if (t == lo) { acc = f; acc_idx = f_idx; continue; }
            // acc *= f (matrix.rs:116-122 `Product`: left to right)
            product_structure(l, acc_idx, f_idx, out_idx, start, pairs);
            const size_t elems = out_idx.size() << log_l;
            double4 *out = nullptr;
            unsigned *d_start = nullptr;
            fhe::LinPair *d_pairs = nullptr;
            if (rc == FHE_OK) {
                err = hipMalloc((void **)&out, elems * sizeof(double4));
                if (err == hipSuccess) err = hipMalloc((void **)&d_start, start.size() * sizeof(unsigned));
                if (err == hipSuccess) err = hipMalloc((void **)&d_pairs, pairs.size() * sizeof(fhe::LinPair));
                if (err == hipSuccess) err = hipMemcpy(d_start, start.data(), start.size() * sizeof(unsigned), hipMemcpyHostToDevice);
                if (err == hipSuccess) err = hipMemcpy(d_pairs, pairs.data(), pairs.size() * sizeof(fhe::LinPair), hipMemcpyHostToDevice);
                if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; }
            }
            if (rc == FHE_OK)
                rc = fhe::launch<fhe::lin_product_kernel>(grid_for(elems), 256, 0, nullptr, (const double4 *)acc, (const double4 *)f, out, (const unsigned *)d_start,
                                                          (const fhe::LinPair *)d_pairs, (unsigned)out_idx.size(), (unsigned)log_l);
            if (hipDeviceSynchronize() != hipSuccess && rc == FHE_OK) rc = FHE_ERR_HIP;
            (void)hipFree(acc); (void)hipFree(f);
            if (d_start) (void)hipFree(d_start);
            if (d_pairs) (void)hipFree(d_pairs);
            acc = out; acc_idx = out_idx;
        }
        p->mats[c].d = acc;
    }
    if (hipDeviceSynchronize() != hipSuccess && rc == FHE_OK) rc = FHE_ERR_HIP;
    return rc;
}

// 5^j mod 2n (`CkksParam::pow5`, ckks.rs:49-51) and the inverse of an odd t mod 2n
unsigned pow5_mod(uint64_t j, size_t n) {
    const uint64_t m = 2 * (uint64_t)n;
    uint64_t r = 1 % m, b = 5 % m;
    for (; j; j >>= 1, b = b * b % m)
        if (j & 1) r = r * b % m;
    return (unsigned)r;
}
unsigned inv_odd(unsigned t, size_t n) {
    uint64_t x = t;  // Newton: doubles the correct low bits, 3 bits to start (t t = 1 mod 8)
    for (int i = 0; i < 5; ++i) x *= 2 - (uint64_t)t * x;
    return (unsigned)(x & (2 * (uint64_t)n - 1));
}

const LinMat *matrix_of(const fhe_ckks_linear_plan *p, int k) { return (p && k >= 0 && k < (int)p->mats.size()) ? &p->mats[k] : nullptr; }
}  // namespace

extern "C" {

void fhe_ckks_linear_plan_destroy(fhe_ckks_linear_plan *p) {
    if (!p) return;
    if (p->device >= 0) {
        DeviceGuard guard(p->device);
        free_mats(p);
    }
    delete p;
}

int fhe_ckks_linear_plan_create(const fhe_ckks_encoder *enc, int r, int inverse, fhe_ckks_linear_plan **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!enc || r < 1) return FHE_ERR_INVALID;
    if (enc->l < 2) return FHE_ERR_UNSUPPORTED;  // n = 2: `sfft_fmats(1)` is the empty list, there is no matrix to apply
    fhe_ckks_linear_plan *p = nullptr;
    try {  // the structure lives in std::vectors: no exception crosses the C boundary
        p = new fhe_ckks_linear_plan();
        p->enc = enc; p->l = enc->l; p->log_l = enc->log_l; p->r = r > enc->log_l ? enc->log_l : r; p->inverse = inverse ? 1 : 0; p->device = enc->device;
        const int depth = (p->log_l + p->r - 1) / p->r;
        p->mats.resize(depth);
        std::vector<uint32_t> f_idx, out_idx;
        std::vector<unsigned> start;
        std::vector<fhe::LinPair> pairs;
        fhe::FactorDiags D{};
        for (int c = 0; c < depth; ++c) {
            LinMat &m = p->mats[c];
            for (int t = c * p->r; t < std::min(p->log_l, (c + 1) * p->r); ++t) {
                factor_diags(p->l, (unsigned)(p->inverse ? p->log_l - 1 - t : t), p->inverse != 0, f_idx, D);
                if (t == c * p->r) { m.idx = f_idx; continue; }
                product_structure(p->l, m.idx, f_idx, out_idx, start, pairs);
                m.idx = out_idx;
            }
            if ((m.idx.size() << p->log_l) > LIN_MAX_ELEMS) { delete p; return FHE_ERR_UNSUPPORTED; }
            bsgs_split(m, p->l);
            for (const std::vector<uint32_t> *v : {&m.giant, &m.baby})
                for (uint32_t x : *v)
                    if (x) p->rot.push_back(x);
        }
        std::sort(p->rot.begin(), p->rot.end());
        p->rot.erase(std::unique(p->rot.begin(), p->rot.end()), p->rot.end());
    } catch (const std::bad_alloc &) {
        delete p;
        return FHE_ERR_INVALID;
    }
    if (p->device >= 0) {
        DeviceGuard guard(p->device);
        int rc = guard.ok ? FHE_OK : FHE_ERR_HIP;
        if (rc == FHE_OK) {
            try { rc = fill_values(p); } catch (const std::bad_alloc &) { rc = FHE_ERR_INVALID; }
        }
        if (rc != FHE_OK) { fhe_ckks_linear_plan_destroy(p); return rc; }
    }
    *out = p;
    return FHE_OK;
}

int fhe_ckks_linear_plan_info(const fhe_ckks_linear_plan *p, int *depth, int *n_rot) {
    if (!p) return FHE_ERR_INVALID;
    if (depth) *depth = (int)p->mats.size();
    if (n_rot) *n_rot = (int)p->rot.size();
    return FHE_OK;
}

int fhe_ckks_linear_plan_rotations(const fhe_ckks_linear_plan *p, uint32_t *out, int count) {
    if (!p || (!out && count) || count < 0 || count > (int)p->rot.size()) return FHE_ERR_INVALID;
    std::copy(p->rot.begin(), p->rot.begin() + count, out);
    return FHE_OK;
}

int fhe_ckks_linear_plan_matrix_info(const fhe_ckks_linear_plan *p, int k, int *n_diag, uint32_t *bsgs_k, int *n_giant, int *n_baby) {
    const LinMat *m = matrix_of(p, k);
    if (!m) return FHE_ERR_INVALID;
    if (n_diag) *n_diag = (int)m->idx.size();
    if (bsgs_k) *bsgs_k = m->k;
    if (n_giant) *n_giant = (int)m->giant.size();
    if (n_baby) *n_baby = (int)m->baby.size();
    return FHE_OK;
}

int fhe_ckks_linear_plan_matrix_split(const fhe_ckks_linear_plan *p, int k, uint32_t *diag, uint32_t *giant, uint32_t *baby, uint8_t *present) {
    const LinMat *m = matrix_of(p, k);
    if (!m) return FHE_ERR_INVALID;
    if (diag) std::copy(m->idx.begin(), m->idx.end(), diag);
    if (giant) std::copy(m->giant.begin(), m->giant.end(), giant);
    if (baby) std::copy(m->baby.begin(), m->baby.end(), baby);
    if (present) std::copy(m->present.begin(), m->present.end(), present);
    return FHE_OK;
}

int fhe_ckks_linear_plan_diags(const fhe_ckks_linear_plan *p, int k, double *out) {
    const LinMat *m = matrix_of(p, k);
    if (!m || !out || p->device < 0 || !m->d) return FHE_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (!guard.ok) return FHE_ERR_HIP;
    HIP_TRY(hipMemcpy(out, m->d, (m->idx.size() << p->log_l) * sizeof(double4), hipMemcpyDeviceToHost));
    return FHE_OK;
}

int fhe_ckks_rtk_gen(const fhe_rns_ctx *r, const uint64_t *sk, size_t n, int64_t j, const fhe_rng *rng, uint64_t stream_id, uint64_t *ksk_b, uint64_t *ksk_a,
                     fhe_mem mem, void *stream) {
    if (!rng || !r || !sk || !ksk_b || !ksk_a || !is_pow2(n) || n < 4) return FHE_ERR_INVALID;
    const int rc0 = fhe::ckks_ring_status(r, n);
    if (rc0 != FHE_OK) return rc0;
    const int64_t l = (int64_t)(n / 2);
    const uint64_t jm = (uint64_t)(((j % l) + l) % l);
    if (jm == 0) return FHE_ERR_INVALID;  // the identity rotation has no key
    if (n >> 31) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(r->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t words = size_t(r->L + r->K) * n;
    Mirror msk(sk, n, mem, true, st), mb(ksk_b, words, mem, false, st), ma(ksk_a, words, mem, false, st);
    if (msk.rc | mb.rc | ma.rc) return FHE_ERR_HIP;
    StreamWs ws(n * sizeof(u64), st);
    if (ws.rc != FHE_OK) return ws.rc;
    FHE_TRY(fhe::launch<fhe::sk_automorphism_kernel>(grid_for(n), 256, 0, st, (const long long *)msk.d, ws.as<long long>(), (unsigned)n,
                                                     inv_odd(pow5_mod(jm, n), n)));
    FHE_TRY(fhe_ckks_ksk_gen(r, (const uint64_t *)msk.d, ws.as<uint64_t>(), n, rng, stream_id, (uint64_t *)mb.d, (uint64_t *)ma.d, FHE_MEM_DEVICE, stream));
    int rc = mb.sync_out(st);
    return rc != FHE_OK ? rc : ma.sync_out(st);
}

void fhe_ckks_linear_transform_destroy(fhe_ckks_linear_transform *t) {
    if (!t) return;
    for (fhe_ckks_diag_matrix *m : t->mats) fhe_ckks_diag_matrix_destroy(m);
    for (fhe_ckks_key *k : t->keys) fhe_ckks_key_destroy(k);
    delete t;
}

int fhe_ckks_linear_transform_prepare(const fhe_ckks_linear_plan *p, const fhe_rns_ctx *const *levels, int n_levels, uint64_t scale, const uint32_t *rot,
                                      const uint64_t *const *ksk_b, const uint64_t *const *ksk_a, int n_rot, fhe_mem mem, fhe_ckks_linear_transform **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    if (!p || !levels || p->device < 0 || scale == 0 || n_rot < 0 || (n_rot && (!rot || !ksk_b || !ksk_a))) return FHE_ERR_INVALID;
    const int depth = (int)p->mats.size();
    if (n_levels < depth + 1) return FHE_ERR_INVALID;
    const fhe_rns_ctx *top = levels[0];
    if (!top || top->device != p->device || top->L < depth + 1) return FHE_ERR_INVALID;
    const size_t n = p->enc->n;
    const int rc0 = fhe::ckks_ring_status(top, n);
    if (rc0 != FHE_OK) return rc0;
    const int L = top->L, K = top->K;
    for (int s = 1; s <= depth; ++s) {  // levels[s]: qs[0 .. L - s) with the same ps on the same device
        const fhe_rns_ctx *c = levels[s];
        if (!c || c->device != top->device || c->L != L - s || c->K != K || c->ps != top->ps) return FHE_ERR_INVALID;
        if (!std::equal(c->qs.begin(), c->qs.end(), top->qs.begin())) return FHE_ERR_INVALID;
    }
    std::map<uint32_t, int> where;  // rotation index mod l -> position in rot
    for (int i = 0; i < n_rot; ++i) {
        if (!ksk_b[i] || !ksk_a[i]) return FHE_ERR_INVALID;
        where[rot[i] % p->l] = i;
    }
    for (uint32_t x : p->rot)
        if (!where.count(x)) return FHE_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (!guard.ok) return FHE_ERR_HIP;
    fhe_ckks_linear_transform *t = new (std::nothrow) fhe_ckks_linear_transform();
    if (!t) return FHE_ERR_INVALID;
    t->device = p->device; t->n = n;
    int rc = FHE_OK;
    uint64_t *key_tmp = nullptr;  // [2][L + K][n]: one key cut down to a level
    std::map<std::pair<int, uint32_t>, fhe_ckks_key *> made;
    // the key of rotation x on levels[s]: rows 0 .. L - s of the q-limbs and all K p-limbs of the caller's key (the reference's key
    // switch at a lower level multiplies on the limbs both sides have, rns.rs:148-158)
    auto key_at = [&](int s, uint32_t x, const fhe_ckks_key **key) -> int {
        *key = nullptr;
        if (x == 0) return FHE_OK;
        const auto it = made.find({s, x});
        if (it != made.end()) { *key = it->second; return FHE_OK; }
        const size_t Ls = size_t(L - s), half = (Ls + K) * n;
        const hipMemcpyKind kind = mem == FHE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const uint64_t *src[2] = {ksk_b[where[x]], ksk_a[where[x]]};
        for (int h = 0; h < 2; ++h) {
            HIP_TRY(hipMemcpy(key_tmp + h * half, src[h], Ls * n * sizeof(u64), kind));
            HIP_TRY(hipMemcpy(key_tmp + h * half + Ls * n, src[h] + size_t(L) * n, size_t(K) * n * sizeof(u64), kind));
        }
        fhe_ckks_key *made_key = nullptr;
        FHE_TRY(fhe_ckks_ksk_prepare(levels[s], key_tmp, key_tmp + half, n, FHE_MEM_DEVICE, &made_key));
        t->keys.push_back(made_key);
        made[{s, x}] = made_key;
        *key = made_key;
        return FHE_OK;
    };
    try {
        t->levels.assign(levels, levels + depth + 1);
        hipError_t err = hipMalloc((void **)&key_tmp, 2 * size_t(L + K) * n * sizeof(uint64_t));
        if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; }
        for (int s = 0; s < depth && rc == FHE_OK; ++s) {  // bootstrapping.rs:87: the matrices last to first
            const LinMat &m = p->mats[depth - 1 - s];
            const fhe_rns_ctx *hi = levels[s], *lo = levels[s + 1];
            std::vector<const fhe_ckks_key *> bk(m.baby.size()), gk(m.giant.size());
            for (size_t j = 0; j < m.baby.size() && rc == FHE_OK; ++j) rc = key_at(s, m.baby[j], &bk[j]);
            for (size_t i = 0; i < m.giant.size() && rc == FHE_OK; ++i) rc = key_at(s + 1, m.giant[i], &gk[i]);
            if (rc != FHE_OK) break;
            // diag_rot(i, j) = diag(i + j).rot_iter(-i) (bootstrapping.rs:101) for the present (i, j), row-major
            std::vector<uint2> terms;
            for (size_t i = 0; i < m.giant.size(); ++i)
                for (size_t j = 0; j < m.baby.size(); ++j)
                    if (m.present[i * m.baby.size() + j]) {
                        const uint32_t d = m.giant[i] + m.baby[j];
                        terms.push_back(uint2{(unsigned)(std::lower_bound(m.idx.begin(), m.idx.end(), d) - m.idx.begin()), m.giant[i] % p->l});
                    }
            uint2 *d_terms = nullptr;
            uint64_t *pt = nullptr;
            err = hipMalloc((void **)&d_terms, terms.size() * sizeof(uint2));
            if (err == hipSuccess) err = hipMalloc((void **)&pt, terms.size() * size_t(hi->L) * n * sizeof(u64));
            if (err == hipSuccess) err = hipMemcpy(d_terms, terms.data(), terms.size() * sizeof(uint2), hipMemcpyHostToDevice);
            if (err != hipSuccess) { g_last_hip = (int)err; rc = FHE_ERR_HIP; }
            // (no entry leaves the encoder's range: |entry| <= 3^r <= 2^23 and scale < 2^64, far below 2^126)
            if (rc == FHE_OK) rc = fhe::ckks_encode_diag_rot(p->enc, hi, scale, fhe::DiagRotIn{m.d, d_terms, p->l}, terms.size(), (u64 *)pt, nullptr);
            if (hipDeviceSynchronize() != hipSuccess && rc == FHE_OK) rc = FHE_ERR_HIP;
            fhe_ckks_diag_matrix *dm = nullptr;
            if (rc == FHE_OK)
                rc = fhe_ckks_diag_matrix_prepare(hi, lo, n, m.giant.data(), (int)m.giant.size(), m.baby.data(), (int)m.baby.size(), m.present.data(), pt, bk.data(),
                                                  gk.data(), FHE_MEM_DEVICE, &dm);
            if (dm) t->mats.push_back(dm);
            if (d_terms) (void)hipFree(d_terms);
            if (pt) (void)hipFree(pt);
        }
    } catch (const std::bad_alloc &) {
        rc = FHE_ERR_INVALID;
    }
    if (key_tmp) (void)hipFree(key_tmp);
    if (rc != FHE_OK) { fhe_ckks_linear_transform_destroy(t); return rc; }
    *out = t;
    return FHE_OK;
}

int fhe_ckks_linear_transform_apply(const fhe_ckks_linear_transform *t, const uint64_t *ct_b, const uint64_t *ct_a, uint64_t *out_b, uint64_t *out_a,
                                    size_t batch, fhe_mem mem, void *stream) {
    if (!t || ((!ct_b || !ct_a || !out_b || !out_a) && batch)) return FHE_ERR_INVALID;
    if (batch == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const size_t n = t->n, depth = t->mats.size(), L = (size_t)t->levels[0]->L;
    if (batch > (size_t(1) << 40) / (L * n)) return FHE_ERR_UNSUPPORTED;
    const size_t in_w = batch * L * n, out_w = batch * (L - depth) * n;
    Mirror mb(ct_b, in_w, mem, true, st), ma(ct_a, in_w, mem, true, st), mob(out_b, out_w, mem, false, st), moa(out_a, out_w, mem, false, st);
    if (mb.rc | ma.rc | mob.rc | moa.rc) return FHE_ERR_HIP;
    // the ciphertexts between the steps: two buffers of the size after step 0, used in turn
    const size_t mid_w = depth > 1 ? batch * (L - 1) * n : 0;
    StreamWs ws(4 * mid_w * sizeof(u64), st);
    if (ws.rc != FHE_OK) return ws.rc;
    const uint64_t *src_b = (const uint64_t *)mb.d, *src_a = (const uint64_t *)ma.d;
    for (size_t s = 0; s < depth; ++s) {
        uint64_t *dst_b = s + 1 == depth ? (uint64_t *)mob.d : ws.as<uint64_t>() + (s & 1) * 2 * mid_w;
        uint64_t *dst_a = s + 1 == depth ? (uint64_t *)moa.d : dst_b + mid_w;
        FHE_TRY(fhe_ckks_mul_mat(t->mats[s], src_b, src_a, dst_b, dst_a, batch, FHE_MEM_DEVICE, stream));
        src_b = dst_b; src_a = dst_a;
    }
    int rc = mob.sync_out(st);
    return rc != FHE_OK ? rc : moa.sync_out(st);
}

}  // extern "C"

namespace fhe {
const std::vector<const fhe_rns_ctx *> &ckks_linear_transform_levels(const fhe_ckks_linear_transform *t, size_t *n) {
    *n = t->n;
    return t->levels;
}
}  // namespace fhe
