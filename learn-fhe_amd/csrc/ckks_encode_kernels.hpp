// Kernels of the CKKS encoder (scheme/ckks/src/ckks.rs:186-213 `Ckks::encode` / `decode`, scheme/ckks/src/sfft.rs:7-72 `sfft` / `sifft`):
// the special FFT over the powers-of-5 ordered roots in double-double arithmetic (dd.hpp), with the encode tail (scale, truncate,
// reduce into the limbs) fused behind `sifft` and the decode head (exact centred lift, round to dd, divide by the scale) fused in
// front of `sfft`.
//
// A complex dd element is 32 bytes (re.hi, re.lo, im.hi, im.lo).  Two kernels serve every size l = 2^log_l:
//   sfft_lds_kernel   log_c <= 12 stages of chunks of C = 2^log_c contiguous elements in LDS (32 C bytes, 128 KiB at C = 4096), one
//                     chunk per workgroup pass; the bit reversal is folded into its global accesses;
//   sfft_top_kernel   the S = log_l - 12 stages above that (half-lengths m >= 4096) on R = 2^S elements per thread in registers,
//                     straight from and to HBM, only for l > 4096.
// `sifft` = top (DIF) -> workspace -> lds (DIF, bit reversal, 1/l);  `sfft` = lds (bit reversal, DIT) -> workspace -> top (DIT).
// Where an element comes from and where it goes is a template argument (ZIn / ZOut / WsIn / WsOut / DecodeHead / EncodeTail), so the
// fused entries run the same two kernels and no intermediate array of slots exists.
//
// Every butterfly performs the operations of dd.hpp's sifft_host / sfft_host on the same values in the same order (the data flow
// of the transform fixes the operands of every butterfly, whatever the schedule), so device and host results have the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "arith.hpp"
#include "ckks_matmul_kernels.hpp"
#include "dd.hpp"
#include "dev_arith.hpp"
#include "rns_kernels.hpp"

namespace fhe {

using ddm::cdd;
using ddm::dd;

constexpr int ENC_MAX_LOG_L = 14;    // l = n / 2 <= 2^14: the cfg4 ring
constexpr int ENC_LDS_LOG_C = 12;    // the largest chunk one workgroup holds: 4096 elements, 128 KiB of the CU's 160 KiB
constexpr int ENC_STATUS_RANGE = 1;  // the encoder's status word: a non-finite value or |z scale| >= 2^126 (encode), a lift beyond f64 (decode)

struct EncTables {
    const double4 *tw;     // [4 l] cis(pi / 2l)^i as (re.hi, re.lo, im.hi, im.lo)
    const unsigned *pow5;  // [max(l / 2, 1)] 5^k mod 4 l
    unsigned log_l;
};

__device__ __forceinline__ cdd unpack(double4 v) { return cdd{dd{v.x, v.y}, dd{v.z, v.w}}; }
__device__ __forceinline__ double4 pack(cdd v) { return double4{v.re.hi, v.re.lo, v.im.hi, v.im.lo}; }

// sfft.rs:46-54: butterfly k of the stage with half-length m = 2^lm uses tw[(+-5^k mod 8m) (4l / 8m)]
__device__ __forceinline__ cdd enc_twiddle(const EncTables &T, unsigned lm, unsigned k, bool conj) {
    const unsigned mask = (8u << lm) - 1;
    unsigned e = T.pow5[k] & mask;
    if (conj) e = ((8u << lm) - e) & mask;
    return unpack(T.tw[(size_t)e << (T.log_l - 1 - lm)]);
}

// ---- where elements come from and go to ------------------------------------------------------------------------------------------
// [msgs][l][2] f64 arrays: the high words (the memory of a complex128 array) and the low words (may be null)
struct ZIn {
    const double2 *hi, *lo;
    unsigned l;
    __device__ __forceinline__ cdd load(size_t msg, unsigned i) const {
        const double2 h = hi[msg * l + i];
        const double2 o = lo ? lo[msg * l + i] : double2{0.0, 0.0};
        return cdd{dd{h.x, o.x}, dd{h.y, o.y}};
    }
};
struct ZOut {
    double2 *hi, *lo;
    unsigned l;
    __device__ __forceinline__ void store(size_t msg, unsigned i, cdd v) const {
        hi[msg * l + i] = double2{v.re.hi, v.im.hi};
        if (lo) lo[msg * l + i] = double2{v.re.lo, v.im.lo};
    }
};
// the workspace between the two passes of l > 4096: [msgs][l] elements
struct WsIn {
    const double4 *w;
    unsigned l;
    __device__ __forceinline__ cdd load(size_t msg, unsigned i) const { return unpack(w[msg * l + i]); }
};
struct WsOut {
    double4 *w;
    unsigned l;
    __device__ __forceinline__ void store(size_t msg, unsigned i, cdd v) const { w[msg * l + i] = pack(v); }
};

// The source of the encode kernels for `diag_rot(i, j)` (bootstrapping.rs:101, ckks_linear_api.hip): message t is diagonal terms[t].x (slot) read at
// (c - terms[t].y) mod l, so the rotation costs nothing and no rotated copy exists.
struct DiagRotIn {
    const double4 *diags;  // [n_diag][l]
    const uint2 *terms;    // [msgs] (slot of diagonal i + j, i mod l)
    unsigned l;
    __device__ __forceinline__ cdd load(size_t msg, unsigned c) const {
        const uint2 t = terms[msg];
        return unpack(diags[(size_t)t.x * l + ((c - t.y) & (l - 1))]);
    }
};

// ckks.rs:191-195: coefficient i <- BigInt::from(z_i.re * scale), coefficient l + i <- BigInt::from(z_i.im * scale), each reduced into
// every limb (`RnsRq::from_bigint`); a negative v gives q - (|v| mod q).
struct EncodeTail {
    u64 *pt;  // [msgs][L][2 l]
    unsigned l, L;
    const Barrett *bar;  // [L]
    const u64 *mu;       // [L] floor(2^64 / q)
    dd scale;
    int *status;
    __device__ __forceinline__ void coeff(size_t msg, unsigned c, dd z) const {
        bool ok;
        const ddm::i128 v = ddm::to_i128(ddm::mul(z, scale), ok);
        if (!ok) atomicOr(status, ENC_STATUS_RANGE);
        const bool negative = v < 0;
        const ddm::u128 mag = negative ? (ddm::u128)0 - (ddm::u128)v : (ddm::u128)v;
        for (unsigned j = 0; j < L; ++j) {
            const Barrett b = bar[j];
            const u64 r = reduce128((u64)mag, (u64)(mag >> 64), b, mu[j]);
            pt[(msg * L + j) * 2 * l + c] = (negative && r) ? b.q - r : r;
        }
    }
    __device__ __forceinline__ void store(size_t msg, unsigned i, cdd v) const {
        coeff(msg, i, v.re);
        coeff(msg, l + i, v.im);
    }
};

// What the decode head needs of the context: Garner's constants c_i = (q_0 .. q_{i-1})^-1 mod q_i and Q = q_0 .. q_{L-1} as words.
struct DecodeConsts {
    u64 q[RNS_MAX_LIMBS], cinv[RNS_MAX_LIMBS], big_q[RNS_MAX_LIMBS];
};

// ckks.rs:203-208: `into_bigint` (the centred lift in (-Q/2, Q/2]) and F256::from(z) / scale, per coefficient.  Mixed radix: digits
// d_i < q_i with v = d_0 + d_1 q_0 + d_2 q_0 q_1 + ..; then v as L words, Q - v where v > floor(Q / 2): integers throughout, so a
// centred value of a few bits comes out exact however large Q is.  M bounds L (the arrays live in registers or scratch).
template <int M>
struct DecodeHead {
    const u64 *pt;  // [msgs][L][2 l]
    unsigned l, L;
    const Barrett *bar;
    const u64 *mu;
    dd scale;
    int *status;
    DecodeConsts K;
    __device__ __forceinline__ dd coeff(size_t msg, unsigned c) const {
        u64 d[M], w[M];
#pragma unroll
        for (int i = 0; i < M; ++i) { d[i] = 0; w[i] = 0; }
        d[0] = pt[(msg * L) * 2 * l + c];
        for (unsigned i = 1; i < L; ++i) {
            const Barrett b = bar[i];
            const u64 m = mu[i];
            u64 t = red64(d[i - 1], m, b.q);  // (d_0 + d_1 q_0 + ..) mod q_i by Horner from the top digit
            for (int j = (int)i - 2; j >= 0; --j) {
                u64 lo = d[j], hi = 0;
                mac128(lo, hi, t, K.q[j]);
                t = reduce128(lo, hi, b, m);
            }
            const u64 x = pt[(msg * L + i) * 2 * l + c];
            d[i] = mulmod_barrett(x >= t ? x - t : x + b.q - t, K.cinv[i], b);
        }
        // v = ((d_{L-1} q_{L-2} + d_{L-2}) q_{L-3} + ..): below Q < 2^(64 L), never a carry out of word L - 1
        w[0] = d[L - 1];
        for (int j = (int)L - 2; j >= 0; --j) {
            u64 carry = d[j];
            const u64 qj = K.q[j];
#pragma unroll
            for (int k = 0; k < M; ++k) {
                u64 lo = carry, hi = 0;
                mac128(lo, hi, w[k], qj);
                w[k] = lo;
                carry = hi;
            }
        }
        // v > floor(Q / 2)?  compared from the top word
        bool above = false, decided = false;
#pragma unroll
        for (int k = M - 1; k >= 0; --k) {
            const u64 half = (K.big_q[k] >> 1) | (k + 1 < M ? K.big_q[k + 1] << 63 : 0ull);
            if (!decided && w[k] != half) { above = w[k] > half; decided = true; }
        }
        if (above) {  // Q - v
            u64 borrow = 0;
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const u64 a = K.big_q[k], s = a - w[k], r = s - borrow;
                borrow = (a < w[k] || s < borrow) ? 1 : 0;
                w[k] = r;
            }
        }
        const dd v = ddm::from_words(w, M, above);
        const dd z = ddm::div(v, scale);
        if (!(std::fabs(z.hi) < __builtin_huge_val())) atomicOr(status, ENC_STATUS_RANGE);
        return z;
    }
    __device__ __forceinline__ cdd load(size_t msg, unsigned i) const { return cdd{coeff(msg, i), coeff(msg, l + i)}; }
};

// ---- the transforms ----------------------------------------------------------------------------------------------------------------
// Stages of half-length m < C = 2^log_c on chunks of C elements in LDS; chunk c of message msg holds elements c C .. c C + C - 1 of
// the stage array.  INV (sifft, DIF, conjugated twiddles, m descending): loads in place, stores element o of the chunk to its
// bit-reversed position rev_12(o) 2^S + rev_S(c) scaled by 1 / l.  Forward (sfft, DIT, m ascending): loads from those positions.
template <bool INV, class Src, class Dst>
__global__ __launch_bounds__(512) void sfft_lds_kernel(Src src, Dst dst, EncTables T, unsigned log_c, size_t chunks) {
    extern __shared__ __attribute__((aligned(32))) unsigned char enc_lds_raw[];
    double4 *lds = reinterpret_cast<double4 *>(enc_lds_raw);
    const unsigned C = 1u << log_c, S = T.log_l - log_c, tid = threadIdx.x, nt = blockDim.x;
    const double inv_l = 1.0 / (double)(1u << T.log_l);
    for (size_t blk = blockIdx.x; blk < chunks; blk += gridDim.x) {
        const size_t msg = blk >> S;
        const unsigned c = (unsigned)(blk & ((size_t(1) << S) - 1)), rc = ddm::bit_rev(c, (int)S);
        for (unsigned t = tid; t < C; t += nt) {
            if (INV) lds[t] = pack(src.load(msg, c * C + t));
            else lds[ddm::bit_rev(t, (int)log_c)] = pack(src.load(msg, (t << S) + rc));
        }
        __syncthreads();
        for (unsigned st = 0; st < log_c; ++st) {
            const unsigned lm = INV ? log_c - 1 - st : st, m = 1u << lm;
            for (unsigned b = tid; b < C / 2; b += nt) {
                const unsigned k = b & (m - 1), i0 = ((b >> lm) << (lm + 1)) + k, i1 = i0 + m;
                cdd x = unpack(lds[i0]), y = unpack(lds[i1]);
                const cdd w = enc_twiddle(T, lm, k, INV);
                if (INV) ddm::dif(x, y, w);
                else ddm::dit(x, y, w);
                lds[i0] = pack(x);
                lds[i1] = pack(y);
            }
            __syncthreads();
        }
        for (unsigned t = tid; t < C; t += nt) {
            if (INV) dst.store(msg, (t << S) + rc, ddm::cmul_pow2(unpack(lds[ddm::bit_rev(t, (int)log_c)]), inv_l));
            else dst.store(msg, c * C + t, unpack(lds[t]));
        }
        __syncthreads();
    }
}

// The S stages of half-length m = l / 2 .. l / 2^S (INV: DIF, descending; forward: DIT, ascending) on R = 2^S elements per thread:
// thread j < l / R of a message holds elements j + t l / R.  Only for l > 4096, where m >= 4096 leaves the chunks of the LDS kernel.
template <bool INV, int S, class Src, class Dst>
__global__ __launch_bounds__(256) void sfft_top_kernel(Src src, Dst dst, EncTables T, size_t msgs) {
    constexpr int R = 1 << S;
    const unsigned log_span = T.log_l - S, span = 1u << log_span;
    const size_t total = msgs << log_span;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t msg = idx >> log_span;
        const unsigned j = (unsigned)(idx & (span - 1));
        cdd x[R];
#pragma unroll
        for (int t = 0; t < R; ++t) x[t] = src.load(msg, j + (unsigned)t * span);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int st = INV ? s : S - 1 - s;        // stage st: m = l >> (st + 1), partners `half` apart in t
            const int half = R >> (st + 1);
            const unsigned lm = T.log_l - 1 - st;
#pragma unroll
            for (int g = 0; g < R; g += 2 * half)
#pragma unroll
                for (int u = 0; u < half; ++u) {
                    const cdd w = enc_twiddle(T, lm, j + (unsigned)u * span, INV);
                    if (INV) ddm::dif(x[g + u], x[g + u + half], w);
                    else ddm::dit(x[g + u], x[g + u + half], w);
                }
        }
#pragma unroll
        for (int t = 0; t < R; ++t) dst.store(msg, j + (unsigned)t * span, x[t]);
    }
}

}  // namespace fhe
