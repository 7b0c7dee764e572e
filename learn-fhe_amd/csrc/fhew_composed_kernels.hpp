// FHEW gadget products and blind rotation at ring sizes the fused kernels of fhew_kernels.hpp do not cover (N = 1 .. 64,
// 4096 .. 2^17), composed from whole-batch launches the way torusk_api.hip's limb_dot composes the torus side:
//   digits kernel -> ntt_fwd_multi -> multiply-accumulate kernel -> ntt_inv_multi -> epilogue
// per gadget product over a chunk of ciphertexts.  Key rows are evaluation-domain rows in the natural order ntt_fwd_multi leaves
// them: [count * rows_per_ct][N] a-components followed by as many b-components.  Every sum is exact mod q, so the outputs are
// bit-identical to the fused kernels' and to the reference's.
#pragma once
#include "fhew_kernels.hpp"

namespace fhe {

// one prepared key set as the composed kernels read it
struct ComposedKey {
    const u64 *rows;  // a rows [count][rows_per_ct][N], the b rows b_off words further
    size_t b_off;
    int rows_per_ct;  // 2d (RGSW) or d (key-switching key)
    DecompParams P;
};

// What every ciphertext of a launch does.  An op is an external product with ep[idx], or (bit BR_OP_AK) a key switch with ks[idx]
// preceded by X -> X^t, t = ak_t[idx] if ak_t else t_fix (1: plain key switch).  ops == nullptr: every ciphertext runs `fixed`;
// otherwise ciphertext c runs ops[c][step], and nothing at all once step >= nops[c] (blind rotation).
struct ComposedOps {
    ComposedKey ep, ks;
    const unsigned *ak_t;
    unsigned t_fix;
    unsigned fixed;
    const unsigned *ops, *nops;
    unsigned max_ops, step;
    size_t ct0;  // index of the launch's first ciphertext in ops / nops
};

__device__ __forceinline__ bool composed_op(const ComposedOps &O, size_t c, unsigned &op) {
    if (!O.ops) { op = O.fixed; return true; }
    const size_t g = O.ct0 + c;
    if (O.step >= O.nops[g]) return false;
    op = O.ops[g * O.max_ops + O.step];
    return true;
}

// t^-1 mod 2N for odd t (Newton: each step doubles the correct low bits, 3 -> 48)
__device__ __forceinline__ unsigned odd_inverse_2n(unsigned t, unsigned n) {
    unsigned x = t;
    for (int k = 0; k < 4; ++k) x *= 2u - t * x;
    return x & (2 * n - 1);
}

// Digits of every ciphertext's RLWE pair (rgsw.rs:116-128: decompose(a) ++ decompose(b); rlwe.rs:177-186: decompose(a) and b kept),
// after X -> X^t (rlwe.rs:188-191) for the key-switch family.  The automorphism is applied as a GATHER through the same index map
// with t^-1 (output j takes +-input auto_target(j, t^-1)): every digit row is written coalesced.
// ct_a, ct_b [chunk][n]; dig [chunk][rows][n]; kept [chunk][n] (key-switch ops: the permuted b).
FHE_HEADER_KERNEL void composed_digits_kernel(const u64 *__restrict__ ct_a, const u64 *__restrict__ ct_b, u64 *__restrict__ dig,
                                              u64 *__restrict__ kept, unsigned n, unsigned rows, size_t chunk, ComposedOps O) {
    const size_t total = size_t(n) * chunk;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t c = idx / n;
        const unsigned j = unsigned(idx - c * n);
        unsigned op;
        if (!composed_op(O, c, op)) continue;
        const bool ks = (op & BR_OP_AK) != 0;
        const unsigned id = op & 0x7fffffffu;
        const DecompParams &P = ks ? O.ks.P : O.ep.P;
        unsigned src = j;
        bool neg = false;
        if (ks) {
            const unsigned t = O.ak_t ? O.ak_t[id] : O.t_fix;
            if (t != 1) src = auto_target(j, odd_inverse_2n(t, n), n, neg);
        }
        u64 va = ct_a[c * n + src], vb = ct_b[c * n + src];
        if (neg) { va = va ? P.q - va : 0; vb = vb ? P.q - vb : 0; }
        u64 *out = dig + c * rows * size_t(n) + j;
        u64 s = decomp_init(va, P);
        for (int r = 0; r < P.d; ++r) out[size_t(r) * n] = decomp_next(s, P);
        if (ks) {
            kept[c * n + j] = vb;
        } else {
            s = decomp_init(vb, P);
            for (int r = 0; r < P.d; ++r) out[size_t(P.d + r) * n] = decomp_next(s, P);
        }
    }
}

// Evaluation-domain multiply-accumulate: acc[c][0 | 1][i] = sum_r dig[c][r][i] * key[idx][r].(a | b)[i] mod q.  V coefficients per
// thread (2: one 16-byte load per operand row, consecutive lanes on consecutive pairs; 1 at N = 1).  Operands are canonical, each
// product is Barrett-reduced without its two final corrections (r < 3q) and folded into a sum kept in [0, q): sum + r < 4q <= 2^64
// since q < 2^62, one canon4 per term, nothing left to reduce at the end.
template <int V>
FHE_HEADER_KERNEL void composed_mac_kernel(const u64 *__restrict__ dig, u64 *__restrict__ acc, unsigned n, unsigned rows, size_t chunk,
                                           ComposedOps O, Barrett B) {
    using Vec = typename std::conditional<V == 2, ulonglong2, u64>::type;
    const unsigned nv = n / V;
    const size_t total = size_t(nv) * chunk;
    const u64 q = B.q, q2 = 2 * q;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t c = idx / nv;
        const unsigned iv = unsigned(idx - c * nv);
        unsigned op;
        if (!composed_op(O, c, op)) continue;
        const bool ks = (op & BR_OP_AK) != 0;
        const ComposedKey &K = ks ? O.ks : O.ep;
        const unsigned id = op & 0x7fffffffu;
        const int nr = ks ? K.P.d : 2 * K.P.d;
        const Vec *x = reinterpret_cast<const Vec *>(dig + c * rows * size_t(n)) + iv;
        const Vec *ka = reinterpret_cast<const Vec *>(K.rows + size_t(id) * K.rows_per_ct * n) + iv;
        const Vec *kb = reinterpret_cast<const Vec *>(K.rows + K.b_off + size_t(id) * K.rows_per_ct * n) + iv;
        u64 sa[V], sb[V];
#pragma unroll
        for (int v = 0; v < V; ++v) sa[v] = sb[v] = 0;
        for (int r = 0; r < nr; ++r) {
            const Vec xv = x[size_t(r) * nv], av = ka[size_t(r) * nv], bv = kb[size_t(r) * nv];
            const u64 *xp = reinterpret_cast<const u64 *>(&xv), *ap = reinterpret_cast<const u64 *>(&av),
                      *bp = reinterpret_cast<const u64 *>(&bv);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                sa[v] = canon4(sa[v] + mulmod_barrett_lazy(xp[v], ap[v], B), q, q2);
                sb[v] = canon4(sb[v] + mulmod_barrett_lazy(xp[v], bp[v], B), q, q2);
            }
        }
        Vec oa, ob;
        u64 *oap = reinterpret_cast<u64 *>(&oa), *obp = reinterpret_cast<u64 *>(&ob);
#pragma unroll
        for (int v = 0; v < V; ++v) { oap[v] = sa[v]; obp[v] = sb[v]; }
        Vec *o = reinterpret_cast<Vec *>(acc + c * 2 * size_t(n));
        o[iv] = oa;
        o[nv + iv] = ob;
    }
}

// (a, b) <- acc (+ the kept b of a key-switch op); ciphertexts without an op this step stay untouched
FHE_HEADER_KERNEL void composed_epilogue_kernel(const u64 *__restrict__ acc, const u64 *__restrict__ kept, u64 *__restrict__ ct_a,
                                                u64 *__restrict__ ct_b, unsigned n, size_t chunk, ComposedOps O, u64 q) {
    const size_t total = size_t(n) * chunk;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t c = idx / n;
        const unsigned j = unsigned(idx - c * n);
        unsigned op;
        if (!composed_op(O, c, op)) continue;
        const u64 *ac = acc + c * 2 * size_t(n);
        ct_a[idx] = ac[j];
        ct_b[idx] = (op & BR_OP_AK) ? csub(ac[n + j] + kept[idx], q) : ac[n + j];
    }
}

// acc = (0, f.automorphism(-g) * X^(b g)) per ciphertext (bootstrapping.rs:164-167), g = 5: the index maps of blind_rotate_kernel
FHE_HEADER_KERNEL void composed_br_init_kernel(const u64 *__restrict__ f, size_t f_stride, const u64 *__restrict__ lwe_b, u64 *__restrict__ out_a,
                                               u64 *__restrict__ out_b, unsigned n, size_t batch, u64 q) {
    const size_t total = size_t(n) * batch;
    const unsigned tneg = (2 * n - 5u) & (2 * n - 1);
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t c = idx / n;
        const unsigned i = unsigned(idx - c * n);
        const unsigned b = unsigned(lwe_b[c] & (2 * n - 1));
        const unsigned kmono = (b * 5u) & (2 * n - 1);
        unsigned pos = unsigned((u64(i) * tneg) & (2 * n - 1));
        pos = (pos + kmono) & (2 * n - 1);
        const u64 v = f[c * f_stride + i];
        out_b[c * n + (pos & (n - 1))] = pos < n ? v : (v ? q - v : 0);
        out_a[idx] = 0;
    }
}

}  // namespace fhe
