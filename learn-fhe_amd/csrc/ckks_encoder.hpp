// The CKKS encoder handle as the extern "C" units share it (ckks_encode_api.hip builds and owns it).
#pragma once
#include <vector>

#include "api_common.hpp"
#include "ckks_encode_kernels.hpp"
#include "dd.hpp"
#include "rns_ctx.hpp"

struct fhe_ckks_encoder {
    size_t n = 0;
    unsigned l = 0;
    int log_l = 0, device = -1;
    std::vector<fhe::cdd> tw;     // [4 l]
    std::vector<unsigned> pow5;   // [max(l / 2, 1)]
    double4 *d_tw = nullptr;
    unsigned *d_pow5 = nullptr;
    int *d_status = nullptr;      // sticky device-side status word: fhe_ckks_encoder_status
};

namespace fhe {
// fhe_ckks_encode on device pointers with the slots read through `src`: pt [msgs][L][n] over rns's qs.  The
// same kernels on the same values as fhe_ckks_encode of the rotated diagonals, so the same bits.  The caller holds the device.
int ckks_encode_diag_rot(const fhe_ckks_encoder *e, const fhe_rns_ctx *rns, uint64_t scale, DiagRotIn src, size_t msgs, u64 *pt, hipStream_t st);
}  // namespace fhe
