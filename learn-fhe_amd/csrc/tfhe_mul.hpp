// Host and device logic of the TGLWE ciphertext product (fhe_tglwe_tensor, fhe_tglwe_relin, fhe_tglwe_mul): plain C++ (no HIP), so that
// it also builds into a stand-alone program.  What is here: the admission rule of a relinearisation gadget, the cut of the tensor's
// second operand, and the closing arithmetic of the tensor -- recombination of the two piece integers and the rounded division.
//
// The tensor needs bits p .. p + 63 of integers sum_i s(x_i) s(y_j) that reach n 2^127 (two such sums for the middle term), where the
// two 60-bit primes recover |value| < p0 p1 / 2 ~ 2^118.9 only.  The second operand is therefore cut, s(y) = hi(y) 2^32 + lo(y) with
// hi signed in [-2^31, 2^31) and lo in [0, 2^32): a sum of n products s(x) hi(y) or s(x) lo(y) stays below n 2^95, the middle term's two
// sums below n 2^96 <= 2^107, inside the n 2^(64 + 33) < 2^118 criterion of torus_kernels.hpp with the piece as the small operand.  Both
// piece integers H and L are recovered as signed 128-bit values and X = H 2^32 + L is formed mod 2^128: rnd_p(X) mod 2^64 reads bits
// p .. p + 63 <= 126 of X + 2^(p - 1) only.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fhe_ring.h"

#if defined(__HIPCC__)
#define FHE_MUL_HD __host__ __device__ inline
#else
#define FHE_MUL_HD inline
#endif

namespace fhe {

// ring and gadget of a relinearisation key: FHE_OK, FHE_ERR_INVALID (a ring the torus context has no transform for) or
// FHE_ERR_UNSUPPORTED (a gadget outside log_b >= 1, d >= 1, log_b d <= 64, d n 2^(64 + log_b) < 2^118)
inline int mul_gadget_check(int log_b, int d, size_t n) {
    if (n != 256 && n != 512 && n != 1024 && n != 2048) return FHE_ERR_INVALID;
    if (log_b < 1 || d < 1 || log_b > 64 || d > 64 || log_b * d > 64) return FHE_ERR_UNSUPPORTED;
    int log_n = 0;
    while ((size_t(1) << log_n) < n) ++log_n;
    const int e = 118 - 64 - log_b - log_n;  // d < 2^e
    if (e <= 0 || (e < 7 && d >= (1 << e))) return FHE_ERR_UNSUPPORTED;
    return FHE_OK;
}

inline int mul_log_delta_check(int log_delta) { return log_delta >= 1 && log_delta <= 63 ? FHE_OK : FHE_ERR_INVALID; }

// s(w) = hi 2^32 + lo
struct MulCut {
    int64_t hi;   // [-2^31, 2^31)
    uint64_t lo;  // [0, 2^32)
};
FHE_MUL_HD MulCut mul_cut(uint64_t w) { return MulCut{(int64_t)w >> 32, w & 0xffffffffull}; }

// a 128-bit integer, two's complement
struct MulWide {
    uint64_t lo, hi;
};

// H 2^32 + L mod 2^128
FHE_MUL_HD MulWide tensor_recombine(MulWide H, MulWide L) {
    MulWide x;
    const uint64_t s_lo = H.lo << 32, s_hi = (H.hi << 32) | (H.lo >> 32);
    x.lo = s_lo + L.lo;
    x.hi = s_hi + L.hi + (x.lo < s_lo ? 1 : 0);
    return x;
}

// floor((X + 2^(p - 1)) / 2^p) mod 2^64 for X given mod 2^128, 1 <= p <= 63
FHE_MUL_HD uint64_t tensor_round(MulWide X, int p) {
    const uint64_t half = uint64_t(1) << (p - 1);
    const uint64_t lo = X.lo + half, hi = X.hi + (lo < half ? 1 : 0);
    return (lo >> p) | (hi << (64 - p));
}

}  // namespace fhe
