// Kernels of the look-up without a padding bit (tfhe_wop_api.hip): the FRONT of a step, the extraction that places a step's rows, and the
// step tables.  All three are element-wise and memory bound; the blind rotation, the key switches, the key fill and the look-up are the
// library's existing kernels behind their public entries.
#pragma once
#include "arith.hpp"
#include "tfhe_wop.hpp"

namespace fhe {

// tab [m][n]: the test polynomial of step l (tfhe_wop.hpp: wop_table_at), the last step's without the correction function
FHE_HEADER_KERNEL void wop_tables_kernel(u64 *__restrict__ tab, unsigned n, int m, int nu, int cb_log_b, int cb_d) {
    const unsigned total = unsigned(m) * n;  // m <= 16, n <= 2048
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int l = int(idx / n);
        tab[idx] = wop_table_at(idx % n, nu, cb_log_b, cb_d, l < m - 1 ? 64 - m + l : -1);
    }
}

// Step front over the batch (n_lwe + 1) words of the remainder, a words first, then the b words.  Per word:
//   rem = src - corr            (corr null in step 0, where src is the caller's input; afterwards src == rem: in place)
//   s   = rem << shift, + 2^62 on a b word
//   a~ / b~ = ((s + half) >> sh) << nu, sh = bits + nu
// which is fhe_tlwe_lincomb {1, -1}, fhe_tlwe_lincomb {2^shift} + 2^62 and fhe_tfhe_mod_switch_many with the remainder read and written
// once.  All arithmetic wraps mod 2^64, as theirs does.
FHE_HEADER_KERNEL void wop_front_kernel(const u64 *src_a, const u64 *src_b, const u64 *__restrict__ cor_a, const u64 *__restrict__ cor_b,
                                        u64 *rem_a, u64 *rem_b, size_t words_a, size_t batch, int shift, int bits, int nu,
                                        u64 *__restrict__ at, u64 *__restrict__ bt) {
    const int sh = bits + nu;  // <= 63: 2^nu <= n / 4
    const u64 half = (u64(1) << sh) >> 1;
    const size_t total = words_a + batch;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const bool is_b = idx >= words_a;
        const size_t i = is_b ? idx - words_a : idx;
        u64 r = is_b ? src_b[i] : src_a[i];
        if (cor_a != nullptr) r -= is_b ? cor_b[i] : cor_a[i];
        (is_b ? rem_b : rem_a)[i] = r;
        const u64 s = (r << shift) + (is_b ? u64(1) << 62 : 0);
        (is_b ? bt : at)[i] = ((s + half) >> sh) << nu;
    }
}

// Extraction and placement of one step: sample_extract(acc_c, e) (tglwe.rs:115-127) for e < cb_d + has_corr with h_e added to the b word.
// Level rows e < cb_d go to lev_a [row][n], lev_b [row], row = c lev_stride + lev_first + e (the [c][l][j] order: lev_stride = m cb_d,
// lev_first = l cb_d); the correction row e = cb_d goes to cx_a [c][n], cx_b [c], where the key switch reads it.
// acc_a, acc_b [batch][n]; one thread per output word, word 0 of a row also writes the row's b.
FHE_HEADER_KERNEL void wop_extract_kernel(const u64 *__restrict__ acc_a, const u64 *__restrict__ acc_b, unsigned n, unsigned batch, int cb_log_b,
                                          int cb_d, int has_corr, int log_delta, size_t lev_stride, size_t lev_first, u64 *__restrict__ lev_a,
                                          u64 *__restrict__ lev_b, u64 *__restrict__ cx_a, u64 *__restrict__ cx_b) {
    const unsigned per = unsigned(cb_d + has_corr);
    const size_t total = size_t(batch) * per * n;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const unsigned j = unsigned(idx % n);
        const size_t re = idx / n;
        const unsigned e = unsigned(re % per);
        const size_t c = re / per;
        const u64 *a = acc_a + c * n;
        const u64 v = j <= e ? a[e - j] : u64(0) - a[n + e - j];
        const bool level = e < unsigned(cb_d);
        const size_t row = level ? c * lev_stride + lev_first + e : c;
        (level ? lev_a : cx_a)[row * n + j] = v;
        if (j == 0) (level ? lev_b : cx_b)[row] = acc_b[c * n + e] + wop_h(int(e), cb_log_b, cb_d, log_delta);
    }
}

}  // namespace fhe
