// Kernels of the CKKS linear transforms (scheme/ckks/src/bootstrapping.rs:23-31 `BootstrappingParam::new`): the factor matrices of
// the special FFT (scheme/ckks/src/sfft.rs:75-99 `sfft_fmats` / `sifft_fmats`), the product of diagonal-sparse matrices
// (util/src/misc/matrix.rs:94-107 `mul_assign`) and the automorphism of an i64 secret key (util/src/avec.rs:34-50) for
// `Ckks::rtk_gen` (scheme/ckks/src/ckks.rs:174-184).  A matrix is its diagonals [n_diag][l] of dd complex elements (32 bytes, the
// encoder's double4 layout); diagonal d holds dense[c][(c + d) mod l] at position c (matrix.rs:87-91).  All three kernels are
// grid-stride loops with one output element per thread and iteration: no atomics, a fixed summation order.
#pragma once
#include <hip/hip_runtime.h>

#include "ckks_encode_kernels.hpp"

namespace fhe {

// Which diagonals of one factor a launch writes.  sfft.rs:79-92 names three vectors: 0 `diag_zero` (index 0), 1 `diag_neg` (index
// l - m), 2 `diag_pos` (index m, absent where log_k == 0).  Slot s of the output holds vector which[s] read at (c - shift[s]) mod l;
// shift is 0 for the forward factor and the vector's own index j for `inv()` (matrix.rs:71-83: index l - j holds
// `rot_iter(l - j)`, that is position c reads c + l - j).
struct FactorDiags {
    int n;
    int which[3];
    unsigned shift[3];
};

// element c of vector `which` of factor log_k: `AVec::broadcast(l, pattern of 2 m)` with m = l >> (1 + log_k); the twiddles are
// `w(2 m)`, read from the encoder's table as the butterflies of half-length m read them
__device__ __forceinline__ cdd factor_value(const EncTables &T, unsigned log_k, int which, unsigned c) {
    const unsigned lm = T.log_l - 1 - log_k, m = 1u << lm, p = c & (2 * m - 1), k = p & (m - 1);
    const bool low = p < m;
    const cdd zero{dd{0.0, 0.0}, dd{0.0, 0.0}}, one{dd{1.0, 0.0}, dd{0.0, 0.0}};
    if (which == 0) {
        if (low) return one;
        const cdd w = enc_twiddle(T, lm, k, false);
        return cdd{ddm::neg(w.re), ddm::neg(w.im)};
    }
    if (which == 1) {
        if (log_k == 0) return low ? enc_twiddle(T, lm, k, false) : one;
        return low ? zero : one;
    }
    return low ? enc_twiddle(T, lm, k, false) : zero;
}

// out [D.n][l]: the diagonals of factor log_k (INV: of its `inv()`: conjugated and halved, halving is exact)
template <bool INV>
__global__ __launch_bounds__(256) void lin_factor_kernel(EncTables T, unsigned log_k, FactorDiags D, double4 *out) {
    const unsigned l = 1u << T.log_l;
    const size_t total = (size_t)D.n << T.log_l;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const unsigned s = (unsigned)(idx >> T.log_l), c = (unsigned)(idx & (l - 1));
        cdd v = factor_value(T, log_k, D.which[s], (c - D.shift[s]) & (l - 1));
        if (INV) v = ddm::cmul_pow2(ddm::cconj(v), 0.5);
        out[idx] = pack(v);
    }
}

// One term of a product: diagonal `a` (slot) of the left matrix, diagonal `b` (slot) of the right one, i = the INDEX of a.
struct LinPair {
    unsigned a, b, i;
};

// matrix.rs:94-107: out[(i + j) mod l][c] = sum over the pairs of that output diagonal of a_i[c] * b_j[(c + i) mod l], the pairs of
// output o being pairs[start[o] .. start[o + 1]) in the reference's order (i ascending, then j ascending).
__global__ __launch_bounds__(256) void lin_product_kernel(const double4 *a, const double4 *b, double4 *out, const unsigned *start, const LinPair *pairs,
                                                          unsigned n_out, unsigned log_l) {
    const unsigned l = 1u << log_l;
    const size_t total = (size_t)n_out << log_l;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const unsigned o = (unsigned)(idx >> log_l), c = (unsigned)(idx & (l - 1));
        const unsigned lo = start[o], hi = start[o + 1];
        LinPair p = pairs[lo];
        cdd acc = ddm::cmul(unpack(a[((size_t)p.a << log_l) + c]), unpack(b[((size_t)p.b << log_l) + ((c + p.i) & (l - 1))]));
        for (unsigned t = lo + 1; t < hi; ++t) {
            p = pairs[t];
            acc = ddm::cadd(acc, ddm::cmul(unpack(a[((size_t)p.a << log_l) + c]), unpack(b[((size_t)p.b << log_l) + ((c + p.i) & (l - 1))])));
        }
        out[idx] = pack(acc);
    }
}

// avec.rs:34-50 `automorphism(t)` of an i64 vector as a gather: out[o] = sk[o t^-1 mod 2n] where that is below n, else
// -sk[o t^-1 mod 2n - n] (t odd: i -> i t mod 2n is a bijection, and (i + n) t = i t + n mod 2n)
__global__ __launch_bounds__(256) void sk_automorphism_kernel(const long long *sk, long long *out, unsigned n, unsigned t_inv) {
    for (size_t o = blockIdx.x * size_t(blockDim.x) + threadIdx.x; o < n; o += size_t(gridDim.x) * blockDim.x) {
        const unsigned i = (unsigned)(((unsigned long long)o * t_inv) & (2ull * n - 1));
        out[o] = i < n ? sk[i] : -sk[i - n];
    }
}

}  // namespace fhe
