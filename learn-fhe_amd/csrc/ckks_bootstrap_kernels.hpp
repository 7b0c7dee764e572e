// Kernels of the CKKS bootstrap glue (csrc/ckks_bootstrap_api.hip): `mod_raise`, the conjugate split after `coeff_to_slot` and the join
// before `slot_to_coeff`.  NO REFERENCE LINE: scheme/ckks/src/bootstrapping.rs stops at the two linear transforms.
//
// All three are element-wise and memory bound.  One thread owns V adjacent coefficients (V = 2: one 16-byte access per limb, taken
// where every pointer is 16-byte aligned and n >= 4; V = 1 otherwise) of one half (b or a) of one ciphertext and walks the limbs:
// consecutive lanes touch consecutive addresses of every limb (coalesced), the per-limb constants are the same for the whole grid and
// come through the constant address space (scalar loads).  No LDS.
//
// The monomial X^(n/2) of the split and the join is an index shift by n/2 with a sign flip on wrap, (X^(n/2) p)[j] = p[j - n/2] for
// j >= n/2 and -p[j + n/2] below; n/2 is even for n >= 4, so a pair of coefficients stays a pair and both carry one sign.
#pragma once
#include "ckks_poly_kernels.hpp"

namespace fhe {

template <int V>
__device__ __forceinline__ void boot_ld(const u64 *p, u64 (&x)[V]) {
    if constexpr (V == 2) {
        const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(p);
        x[0] = t.x; x[1] = t.y;
    } else {
        x[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void boot_st(u64 *p, const u64 (&x)[V]) {
    if constexpr (V == 2) *reinterpret_cast<ulonglong2 *>(p) = ulonglong2{x[0], x[1]};
    else *p = x[0];
}
__device__ __forceinline__ u64 boot_add(u64 x, u64 y, u64 q) { return csub(x + y, q); }
__device__ __forceinline__ u64 boot_sub(u64 x, u64 y, u64 q) { return x >= y ? x - y : x + q - y; }

// in_b, in_a [batch][in_limbs][n], only limb 0 (mod q_0 = B[0].q) is read -> out_b, out_a [batch][L][n]: the centred integer
// v in (-q_0 / 2, q_0 / 2] of every residue, reduced into every limb.  |v| <= q_0 / 2 may exceed a smaller q_l many times over (a 60-bit
// q_0 over 30-bit limbs), so |v| goes through the 64-bit Barrett reduction (red_mu[l] = floor(2^64 / q_l), any 64-bit input) and a
// negative value becomes q_l - (|v| mod q_l), 0 staying 0.
template <int V>
__global__ void ckks_mod_raise_kernel(const u64 *__restrict__ in_b, const u64 *__restrict__ in_a, unsigned in_limbs, u64 *__restrict__ out_b,
                                      u64 *__restrict__ out_a, unsigned n, int L, size_t batch, const Barrett *__restrict__ B, const u64 *__restrict__ red_mu) {
    const size_t row = n / V, half = row * batch, total = 2 * half;
    const u64 q0 = ldc(&B[0].q, 0), top = q0 >> 1;  // q_0 is odd: the non-negative values are 0 .. (q_0 - 1) / 2
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const bool half_a = idx >= half;
        const size_t e = half_a ? idx - half : idx, p = e / row, i = (e - p * row) * V;
        u64 v[V], r[V];
        boot_ld<V>((half_a ? in_a : in_b) + p * in_limbs * n + i, v);
        bool neg[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            neg[k] = v[k] > top;
            if (neg[k]) v[k] = q0 - v[k];
        }
        u64 *out = (half_a ? out_a : out_b) + p * size_t(L) * n + i;
        for (int l = 0; l < L; ++l) {
            const u64 q = ldc(&B[l].q, 0), mu = ldc(red_mu, l);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const u64 m = poly_red64(v[k], mu, q);
                r[k] = neg[k] && m ? q - m : m;
            }
            boot_st<V>(out + size_t(l) * n, r);
        }
    }
}

// ct = (ct_b, ct_a) and its key-switched conjugate cj = (cj_b, cj_a), each [batch][L][n] per half -> out_b, out_a [2 batch][L][n]:
// rows [0, batch) hold R = ct + cj, rows [batch, 2 batch) hold J = -X^(n/2) (ct - cj).  The thread of source coefficient i writes R[i]
// and J[(i + n/2) mod n]: below n/2 that is cj[i] - ct[i], from n/2 on it wraps and is ct[i] - cj[i] -- the shift rides on the store.
template <int V>
__global__ void ckks_conj_split_kernel(const u64 *__restrict__ ct_b, const u64 *__restrict__ ct_a, const u64 *__restrict__ cj_b, const u64 *__restrict__ cj_a,
                                       u64 *__restrict__ out_b, u64 *__restrict__ out_a, unsigned n, int L, size_t batch, const Barrett *__restrict__ B) {
    const size_t row = n / V, half = row * batch, total = 2 * half, h = n / 2;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const bool half_a = idx >= half;
        const size_t e = half_a ? idx - half : idx, p = e / row, i = (e - p * row) * V;
        const u64 *ct = (half_a ? ct_a : ct_b) + p * size_t(L) * n + i, *cj = (half_a ? cj_a : cj_b) + p * size_t(L) * n + i;
        u64 *out = half_a ? out_a : out_b;
        const bool wrap = i >= h;  // V == 2 has n >= 4: both coefficients lie on one side of n/2
        u64 *out_r = out + p * size_t(L) * n + i, *out_j = out + (batch + p) * size_t(L) * n + (wrap ? i - h : i + h);
        for (int l = 0; l < L; ++l) {
            const u64 q = ldc(&B[l].q, 0);
            u64 x[V], y[V], s[V], d[V];
            boot_ld<V>(ct + size_t(l) * n, x);
            boot_ld<V>(cj + size_t(l) * n, y);
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = boot_add(x[k], y[k], q);
            boot_st<V>(out_r + size_t(l) * n, s);
#pragma unroll
            for (int k = 0; k < V; ++k) d[k] = wrap ? boot_sub(x[k], y[k], q) : boot_sub(y[k], x[k], q);
            boot_st<V>(out_j + size_t(l) * n, d);
        }
    }
}

// the inverse layout: in_b, in_a [2 batch][L][n] (rows [0, batch) = R', rows [batch, 2 batch) = J') -> out_b, out_a [batch][L][n] =
// R' + X^(n/2) J'.  The thread of output coefficient j reads J'[(j + n/2) mod n]: from n/2 on that is J'[j - n/2] added, below it is
// J'[j + n/2] subtracted -- the shift rides on the load.
template <int V>
__global__ void ckks_conj_join_kernel(const u64 *__restrict__ in_b, const u64 *__restrict__ in_a, u64 *__restrict__ out_b, u64 *__restrict__ out_a, unsigned n,
                                      int L, size_t batch, const Barrett *__restrict__ B) {
    const size_t row = n / V, half = row * batch, total = 2 * half, h = n / 2;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const bool half_a = idx >= half;
        const size_t e = half_a ? idx - half : idx, p = e / row, j = (e - p * row) * V;
        const u64 *in = half_a ? in_a : in_b;
        u64 *out = (half_a ? out_a : out_b) + p * size_t(L) * n + j;
        const bool upper = j >= h;
        const u64 *in_r = in + p * size_t(L) * n + j, *in_j = in + (batch + p) * size_t(L) * n + (upper ? j - h : j + h);
        for (int l = 0; l < L; ++l) {
            const u64 q = ldc(&B[l].q, 0);
            u64 x[V], y[V], s[V];
            boot_ld<V>(in_r + size_t(l) * n, x);
            boot_ld<V>(in_j + size_t(l) * n, y);
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = upper ? boot_add(x[k], y[k], q) : boot_sub(x[k], y[k], q);
            boot_st<V>(out + size_t(l) * n, s);
        }
    }
}

// avec.rs:34-50 `automorphism(-1)` of an i64 vector (scheme/ckks/src/ckks.rs:169-172 `cjk_gen`): X^i -> X^(-i) = -X^(n - i), so
// out[0] = sk[0] and out[o] = -sk[n - o]
FHE_HEADER_KERNEL void ckks_sk_conj_kernel(const long long *__restrict__ sk, long long *__restrict__ out, unsigned n) {
    for (size_t o = blockIdx.x * size_t(blockDim.x) + threadIdx.x; o < n; o += size_t(gridDim.x) * blockDim.x) out[o] = o ? -sk[n - o] : sk[0];
}

}  // namespace fhe
