// Private functional key switch TLWE -> TGLWE (the second half of the circuit bootstrap of Chillotti-Gama-Georgieva-Izabachene, over
// tlwe.rs:144-153's digit x key product and tglwe.rs:91-103's ciphertexts) as a tiled matrix product over Z/2^64:
//   out(r, u)[half][k] = sum_j sum_i digit_j(c_i) * key[j (n_in + 1) + i][u][half][k],   c = (ct_a[r][0 .. n_in - 1], ct_b[r])
// One key row is W = n_funcs * 2 * n contiguous words, so the product is [batch] x [d (n_in + 1)] digits against [d (n_in + 1)] x [W]
// key words.  A block owns TILE input ciphertexts (grid x), a strip of PFKS_THREADS * VEC key columns over all functions (grid y) and
// every gridDim.z-th chunk of `chunk` input coefficients, all d digits of each (grid z; a chunk's digit image stays below 48 KiB):
//   * the digits of its tile and chunk are computed ONCE into LDS, [d][chunk][TILE]: bytes with +128 when log_b <= 7 (a digit lies in
//     [-64, 64]), so that a term is one v_mad_u64_u32 per output dword; the offset leaves as 128 x (the column sum of the key), which
//     the thread collects while it streams the column.  32-bit signed words otherwise (log_b <= 31).
//   * a thread owns VEC adjacent columns (VEC = 2: one 16-byte load per key row) and keeps 2 * TILE dwords of sums per column; the
//     digits of a row arrive as ONE LDS broadcast read (16 bytes at TILE = 16).
//   * a key word fetched from HBM or L2 serves TILE ciphertexts: the key is streamed ceil(batch / TILE) times.
//   * grid z == 1: plain stores.  grid z > 1 (few tiles: the grid would not fill the chip): partial sums are added with 64-bit
//     atomics into outputs that are ZERO before the launch -- additions mod 2^64 commute, so the bits are those of the plain route.
// Output row of (r, u): ((r / group) * n_funcs + u) * group + r % group (tfhe_cbs.hpp: pfks_out_row).
#pragma once
#include "dispatch.hpp"  // launch(), with_int()
#include "torus_kernels.hpp"
#include "tfhe_cbs.hpp"

namespace fhe {

constexpr int PFKS_THREADS = 128;

struct PfksShape {
    unsigned n_in, n, n_funcs, group, batch, chunk;
    size_t row_words;  // W
};

// plaintext rows of the key (fhe_tlwe_pfksk_gen): pt[(j (n_in + 1) + i) n_funcs + u][k] = w_i g_j F_u[k], w_i = -sk_in[i], w_{n_in} = 1
FHE_HEADER_KERNEL void pfksk_plain_kernel(const u64 *__restrict__ sk_in, const u64 *__restrict__ funcs, u64 *__restrict__ pt, size_t n_in, size_t n,
                                          size_t n_funcs, int d, int rb, int log_b) {
    const size_t total = size_t(d) * (n_in + 1) * n_funcs * n;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t k = idx % n, t = idx / n, u = t % n_funcs, row = t / n_funcs, i = row % (n_in + 1), j = row / (n_in + 1);
        const u64 w = i < n_in ? u64(0) - sk_in[i] : u64(1);
        pt[idx] = (w << (rb + int(j) * log_b)) * funcs[u * n + k];
    }
}

// a, b [rows][n] -> key [rows][2][n]: the two halves of every ciphertext side by side
FHE_HEADER_KERNEL void pfksk_pack_kernel(const u64 *__restrict__ a, const u64 *__restrict__ b, u64 *__restrict__ key, size_t rows, size_t n) {
    const size_t total = 2 * rows * n;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t k = idx % n, t = idx / n, half = t & 1, r = t >> 1;
        key[idx] = (half ? b : a)[r * n + k];
    }
}

// the test polynomial of the circuit bootstrap on the device: tfhe_cbs.hpp's cbs_table_at, coefficient by coefficient
FHE_HEADER_KERNEL void cbs_table_kernel(u64 *__restrict__ out, unsigned n, int nu, int cb_log_b, int cb_d) {
    for (unsigned c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) out[c] = cbs_table_at(c, n, nu, cb_log_b, cb_d);
}

template <int TILE, bool BYTES>
__device__ __forceinline__ void pfks_load_digits(const unsigned char *p, unsigned (&dg)[TILE]) {
    if constexpr (BYTES) {
        if constexpr (TILE % 16 == 0) {
#pragma unroll
            for (int q = 0; q < TILE / 16; ++q) {
                const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int c = 0; c < 16; ++c) dg[16 * q + c] = (w[c >> 2] >> (8 * (c & 3))) & 0xffu;
            }
        } else if constexpr (TILE == 4) {
            const unsigned v = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
            for (int c = 0; c < 4; ++c) dg[c] = (v >> (8 * c)) & 0xffu;
        } else {
#pragma unroll
            for (int c = 0; c < TILE; ++c) dg[c] = p[c];
        }
    } else {
        const unsigned *w = reinterpret_cast<const unsigned *>(p);
        if constexpr (TILE % 4 == 0) {
#pragma unroll
            for (int q = 0; q < TILE / 4; ++q) {
                const uint4 v = reinterpret_cast<const uint4 *>(w)[q];
                dg[4 * q] = v.x; dg[4 * q + 1] = v.y; dg[4 * q + 2] = v.z; dg[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < TILE; ++c) dg[c] = w[c];
        }
    }
}

// dynamic LDS: d * chunk * TILE * (BYTES ? 1 : 4) bytes.  VEC = 2 needs n even and key, out_a, out_b 16-byte aligned.
template <int TILE, int VEC, bool BYTES>
__global__ __launch_bounds__(PFKS_THREADS) void tlwe_pfks_kernel(const u64 *__restrict__ ct_a, const u64 *__restrict__ ct_b, const u64 *__restrict__ key,
                                                                 PfksShape S, TDecomp P, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr unsigned DW = BYTES ? 1u : 4u;  // bytes of a digit
    const unsigned ct0 = blockIdx.x * TILE, rows_in = S.n_in + 1;
    const size_t col = (size_t(blockIdx.y) * PFKS_THREADS + threadIdx.x) * VEC;
    const bool active = col < S.row_words;  // a thread past the last column only keeps the barriers
    u64 acc[VEC][TILE], ksum[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        ksum[v] = 0;
#pragma unroll
        for (int c = 0; c < TILE; ++c) acc[v][c] = 0;
    }
    // the chunks of this block: blockIdx.z, blockIdx.z + gridDim.z, ... (uniform per block)
    for (unsigned i0 = blockIdx.z * S.chunk; i0 < rows_in; i0 += gridDim.z * S.chunk) {
        const unsigned ni = min(S.chunk, rows_in - i0);
        __syncthreads();  // the previous chunk's digits are read
        for (unsigned idx = threadIdx.x; idx < ni * TILE; idx += PFKS_THREADS) {
            const unsigned c = idx / ni, ii = idx - c * ni, i = i0 + ii;
            const bool live = ct0 + c < S.batch;
            u64 st = 0;
            if (live) st = tdecomp_init(i < S.n_in ? ct_a[size_t(ct0 + c) * S.n_in + i] : ct_b[ct0 + c], P);
            for (int j = 0; j < P.d; ++j) {
                const int dg = live ? (int)(long long)tdecomp_next(st, P) : 0;
                const size_t at = (size_t(j) * S.chunk + ii) * TILE + c;
                if constexpr (BYTES) smem_raw[at] = (unsigned char)(128 + dg);
                else reinterpret_cast<int *>(smem_raw)[at] = dg;
            }
        }
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < P.d; ++j) {
            const u64 *kr = key + (size_t(j) * rows_in + i0) * S.row_words + col;
            const unsigned char *dj = smem_raw + size_t(j) * S.chunk * TILE * DW;
#pragma unroll 2
            for (unsigned ii = 0; ii < ni; ++ii) {
                u64 kv[VEC];
                if constexpr (VEC == 2) {
                    const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(kr + size_t(ii) * S.row_words);
                    kv[0] = t.x; kv[1] = t.y;
                } else {
                    kv[0] = kr[size_t(ii) * S.row_words];
                }
                unsigned dg[TILE];
                pfks_load_digits<TILE, BYTES>(dj + size_t(ii) * TILE * DW, dg);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if constexpr (BYTES) {
                        ksum[v] += kv[v];
                        const unsigned klo = (unsigned)kv[v], khi = (unsigned)(kv[v] >> 32);
#pragma unroll
                        for (int c = 0; c < TILE; ++c) {
                            const u64 t = (u64)klo * dg[c] + acc[v][c];                    // the carry rides into the high dword
                            const unsigned hi = khi * dg[c] + (unsigned)(t >> 32);
                            acc[v][c] = ((u64)hi << 32) | (unsigned)t;
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < TILE; ++c) acc[v][c] += kv[v] * (u64)(long long)(int)dg[c];
                    }
                }
            }
        }
    }
    if (!active) return;
    const bool split = gridDim.z > 1;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const size_t w = col + v;
        const unsigned u = (unsigned)(w / (2 * size_t(S.n)));
        const unsigned rem = (unsigned)(w - size_t(u) * 2 * S.n);
        const bool half = rem >= S.n;
        const unsigned k = half ? rem - S.n : rem;
        u64 *base = half ? out_b : out_a;
        const u64 off = BYTES ? ksum[v] << 7 : 0;  // 128 x the column sum
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const unsigned r = ct0 + c;
            if (r >= S.batch) continue;
            const size_t orow = (size_t(r / S.group) * S.n_funcs + u) * S.group + r % S.group;
            u64 *dst = base + orow * S.n + k;
            const u64 val = acc[v][c] - off;
            if (split) atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)val);
            else *dst = val;
        }
    }
}

}  // namespace fhe
