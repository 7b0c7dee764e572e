// Host logic of the circuit bootstrap (fhe_tfhe_circuit_bootstrap, fhe_tlwe_pfks, fhe_tlwe_pfksk_gen): plain C++ (no HIP), so that it
// also builds into a stand-alone program.  What is here: the gadget values, nu = ceil(log2 cb_d), the interleaved test polynomial, the
// output-row mapping of the private functional key switch, the workspace of the fused entry and every argument check that needs no
// device.
//
// The circuit bootstrap turns a TLWE encryption of a bit (pt = bit << 62) into the 2 d rows of a TGGSW encryption of that bit
// (tggsw.rs:79-88): one many-LUT blind rotation (bootstrapping.rs:84-96) whose table holds g_j on n/4 <= c < 3n/4 for level j, an
// extraction per level (tglwe.rs:115-127), and a private functional key switch that multiplies the phase of every extracted TLWE by
// F_0 = -S (rows 0 .. d - 1) and F_1 = 1 (rows d .. 2d - 1).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fhe_ring.h"
#include "tfhe_circuit.hpp"  // TfheScratch

namespace fhe {

constexpr int CBS_MAX_D = 16;         // levels of the output gadget: 2^nu <= 16 tables from one rotation
constexpr int PFKS_MAX_FUNCS = 4;     // functions of one key-switch key
constexpr int PFKS_MAX_LOG_B = 31;    // a digit is kept as a 32-bit word at most

// Base2Decomposor::<T64>::new(log_b, d) is admitted (decompose.rs:66-81)
inline bool cbs_gadget_ok(int log_b, int d) { return log_b >= 1 && log_b <= 63 && d >= 1 && d <= 64 && log_b * d <= 64; }

// g_j = 2^(64 - log_b d + j log_b), j < d: the weight of digit j
inline uint64_t cbs_gadget(int log_b, int d, int j) { return uint64_t(1) << (64 - log_b * d + j * log_b); }

// nu = ceil(log2 cb_d): the rotation serves 2^nu tables, those of j >= cb_d are zero
inline int cbs_nu(int cb_d) {
    int nu = 0;
    while ((1 << nu) < cb_d) ++nu;
    return nu;
}

inline bool cbs_pow2(size_t n) { return n && !(n & (n - 1)); }

// the shape checks of the circuit bootstrap that need no device: FHE_OK, FHE_ERR_INVALID or FHE_ERR_UNSUPPORTED
inline int cbs_check(int cb_log_b, int cb_d, size_t n) {
    if (cb_d < 1 || cb_d > CBS_MAX_D || !cbs_gadget_ok(cb_log_b, cb_d) || !cbs_pow2(n)) return FHE_ERR_INVALID;
    // a quarter of the ring holds whole groups of 2^nu coefficients.  Every admitted ring passes (n / 4 >= 64 >= 2^nu); the check
    // stands for the definition and fails for instance at n = 32 with cb_d = 16 (n / 4 = 8, 2^nu = 16)
    if (n < 4 || (n / 4) % (size_t(1) << cbs_nu(cb_d))) return FHE_ERR_INVALID;
    if (n < 256 || n > 2048) return FHE_ERR_UNSUPPORTED;  // what fhe_tggsw_prepare admits
    return FHE_OK;
}

// Coefficient c of the test polynomial, P[c] = T_{c mod 2^nu}[c - c mod 2^nu], T_j[c] = g_j for n/4 <= c < 3n/4 and j < cb_d, else 0:
// the one statement of the table, for the host (cbs_table) and for the kernel that fills it on the device (pfks_kernels.hpp)
#if defined(__HIPCC__)
#define FHE_CBS_HD __host__ __device__
#else
#define FHE_CBS_HD
#endif
FHE_CBS_HD inline uint64_t cbs_table_at(size_t c, size_t n, int nu, int cb_log_b, int cb_d) {
    const size_t j = c & ((size_t(1) << nu) - 1), base = c - j;
    return (j < (size_t)cb_d && base >= n / 4 && base < 3 * (n / 4)) ? uint64_t(1) << (64 - cb_log_b * cb_d + (int)j * cb_log_b) : 0;
}

// The test polynomial.  out [n].
inline int cbs_table(int cb_log_b, int cb_d, size_t n, uint64_t *out) {
    if (!out) return FHE_ERR_INVALID;
    const int rc = cbs_check(cb_log_b, cb_d, n);
    if (rc != FHE_OK) return rc;
    const int nu = cbs_nu(cb_d);
    for (size_t c = 0; c < n; ++c) out[c] = cbs_table_at(c, n, nu, cb_log_b, cb_d);
    return FHE_OK;
}

// the output row of (input r, function u) of fhe_tlwe_pfks: inputs come in groups of `group`, a group's rows of one function stay together
inline size_t pfks_out_row(size_t r, size_t u, size_t n_funcs, size_t group) { return ((r / group) * n_funcs + u) * group + r % group; }

// words of one key row: the n_funcs (a, b) pairs side by side
inline size_t pfks_row_words(size_t n_funcs, size_t n) { return n_funcs * 2 * n; }
// words of a whole key: d (n_in + 1) rows
inline size_t pfksk_words(int d, size_t n_in, size_t n_funcs, size_t n) { return size_t(d) * (n_in + 1) * pfks_row_words(n_funcs, n); }

// the argument checks of fhe_tlwe_pfks that need no device
inline int pfks_check(int log_b, int d, int n_funcs, size_t n_in, size_t n, size_t group, size_t batch) {
    if (!cbs_gadget_ok(log_b, d) || n_funcs < 1 || n_funcs > PFKS_MAX_FUNCS || n_in == 0 || n == 0 || group == 0) return FHE_ERR_INVALID;
    if (batch % group) return FHE_ERR_INVALID;
    if (log_b > PFKS_MAX_LOG_B) return FHE_ERR_UNSUPPORTED;
    if (n_in >= (size_t(1) << 31) - 1 || n > (size_t(1) << 20) || batch > 0x7fffffffull / (size_t)n_funcs) return FHE_ERR_UNSUPPORTED;
    return FHE_OK;
}

// Stream-ordered scratch of fhe_tfhe_circuit_bootstrap in 64-bit words (tfhe_circuit.hpp: TfheScratch): batch blind rotations, batch cb_d
// extracted TLWEs, no wire table.  The key switch adds none: it reads the extracted rows and writes the caller's output.
inline TfheScratch cbs_scratch(size_t n, size_t n_lwe, int cb_d, size_t batch) { return TfheScratch(batch, batch * size_t(cb_d), n, n_lwe, 0, false); }
inline size_t cbs_workspace(size_t n, size_t n_lwe, int cb_d, size_t batch) { return cbs_scratch(n, n_lwe, cb_d, batch).total; }

}  // namespace fhe
