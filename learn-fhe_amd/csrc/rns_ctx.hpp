// The RNS context and the prepared CKKS key as the extern "C" units share them (rns_api.hip builds and owns them).
#pragma once
#include <vector>

#include "api_common.hpp"
#include "ctx.hpp"
#include "rns_kernels.hpp"

struct fhe_rns_ctx {
    int L = 0, K = 0, device = -1;
    std::vector<uint64_t> qs, ps;
    std::vector<fhe_ctx *> mods;       // L + K per-prime transform contexts (qs then ps)
    fhe::ModDesc *d_descs = nullptr;   // [L + K]
    fhe::Barrett *d_barrett = nullptr; // [L + K]
    void *d_blob = nullptr;            // all conversion tables
    fhe::BaseConv q2p{}, p2q{};
    fhe::RescaleConsts resc{};
    fhe::RescaleConsts resc_last{};    // `rescale()` = rescale_k(1) of a polynomial over qs: drops q_{L-1} (L >= 2)
    int max_log_n = 0;                 // largest ring degree every prime supports
    int all_pm = -1;                   // common pseudo-Mersenne bit length of all primes, 0 if none
    // every modulus a pseudo-Mersenne prime of ONE bit length: the conversions run as unreduced dot products (rns_kernels.hpp)
    bool pm = false;
    fhe::pd::Uni uni{};
    fhe::PmSrc s_q2p{}, s_p2q{}, s_p2q_sum{}, s_p2q_diff{}, s_last{}, s_p2q_plain{};
    fhe::PmRows r_q2p{}, r_q2p_w{}, r_resc{}, r_resc_edge{}, r_last{}, r_p2q_plain{};
};

struct fhe_ckks_key {
    const fhe_rns_ctx *rns = nullptr;
    int log_n = 0;
    u64 *d_kb = nullptr, *d_ka = nullptr;  // [L + K][n], evaluation domain
};

namespace fhe {
// scheme/ckks/src/ckks.rs:284-293 on device pointers (rns_api.hip key_switch_dev): out_b = rescale_K(ksk.b * a~) + add_b,
// out_a = rescale_K(ksk.a * a~) + add_a over [batch][L][n]; addends may be null, outputs may alias the addends and a_in
int ckks_key_switch_dev(const fhe_rns_ctx *r, const fhe_ckks_key *key, const u64 *a_in, const u64 *add_b, const u64 *add_a, u64 *out_b, u64 *out_a,
                        size_t batch, hipStream_t st);
// FHE_OK if a CKKS ring of degree n exists over every modulus of r on a device (rns_api.hip ckks_ring_ok)
int ckks_ring_status(const fhe_rns_ctx *r, size_t n);
// rns.rs:99-101 `rescale()` on device pointers (rns_api.hip, what fhe_rns_rescale launches): in [batch][L][n] -> out [batch][L-1][n]
int ckks_rescale_last_dev(const fhe_rns_ctx *r, const u64 *in, u64 *out, size_t n, size_t batch, hipStream_t st);
// ext [batch][L+K][n] = in || extend_bases(in) (in [batch][L][n]; rns_api.hip launch_extend as the key switch calls it) and
// fhe_rns_rescale_k on device pointers (in [batch][L+K][n] -> out [batch][L][n]): what ckks_hoist_api.hip lifts and lowers with
int ckks_extend_dev(const fhe_rns_ctx *r, const u64 *in, u64 *ext, size_t n, size_t batch, hipStream_t st);
int ckks_rescale_k_dev(const fhe_rns_ctx *r, const u64 *in, u64 *out, size_t n, size_t batch, hipStream_t st);
// the borrowed level chain of a prepared linear transform (ckks_linear_api.hip) or polynomial evaluator (ckks_poly_api.hip), depth + 1
// contexts with levels[0] the input's, and its ring degree: what fhe_ckks_bootstrap_prepare checks its stages against
const std::vector<const fhe_rns_ctx *> &ckks_linear_transform_levels(const fhe_ckks_linear_transform *t, size_t *n);
const std::vector<const fhe_rns_ctx *> &ckks_poly_eval_levels(const fhe_ckks_poly_eval *ev, size_t *n);
}  // namespace fhe
