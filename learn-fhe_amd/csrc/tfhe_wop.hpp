// Host logic of the look-up without a padding bit (fhe_tfhe_wop_table, _workspace, _selectors, _pbs): plain C++ (no HIP), so that it
// also builds into a stand-alone program.  What is here: nu = ceil(log2(cb_d + 1)), the half gadget values h_j, the test polynomial of a
// step, the row order [c][l][j] of the level rows, the workspace and every argument check that needs no device.
//
// A TLWE ciphertext with phase x << (64 - m), 0 <= x < 2^m and NO padding bit, is split into its m bits, least significant first.  Step l
// shifts the running remainder so that bit l stands at 2^63, adds 2^62 and blind-rotates ONE test polynomial all of whose interleaved
// functions are constants: P[c] = -h_{c mod 2^nu}.  Coefficient 0 of v X^(-c~) is v[c~] for c~ < n and -v[c~ - n] above
// (bootstrapping.rs:84-96), so extraction j has phase -h_j for bit 0 and +h_j for bit 1; adding h_j gives bit * 2 h_j.  With h_j = g_j / 2
// (j < cb_d) those are the rows the circuit bootstrap hands to its private functional key switch; with h_{cb_d} = 2^(delta_l - 1) it is
// the bit at its own position, which a key switch brings back to the small key as the next step's correction.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fhe_ring.h"
#include "tfhe_cbs.hpp"  // the gadget, cbs_pow2, TfheScratch

namespace fhe {

constexpr int WOP_MAX_BITS = 16;  // message bits: a table of at most 2^16 entries

// nu = ceil(log2(cb_d + 1)): cb_d level functions and the correction function share one rotation
inline int wop_nu(int cb_d) {
    int nu = 0;
    while ((1 << nu) < cb_d + 1) ++nu;
    return nu;
}

// torus position of bit l of an m-bit message
inline int wop_log_delta(int m, int l) { return 64 - m + l; }

#if defined(__HIPCC__)
#define FHE_WOP_HD __host__ __device__
#else
#define FHE_WOP_HD
#endif
// h_j: g_j / 2 of (cb_log_b, cb_d) for j < cb_d; 2^(log_delta - 1) for j = cb_d (log_delta < 0: the last step, no correction: 0); 0 above.
// cb_log_b cb_d <= 63 keeps g_0 / 2 a whole word.  The one statement, for the host and for the kernels (tfhe_wop_kernels.hpp).
FHE_WOP_HD inline uint64_t wop_h(int j, int cb_log_b, int cb_d, int log_delta) {
    if (j < cb_d) return uint64_t(1) << (63 - cb_log_b * cb_d + j * cb_log_b);
    return (j == cb_d && log_delta >= 1) ? uint64_t(1) << (log_delta - 1) : 0;
}
// coefficient c of a step's test polynomial: -h_{c mod 2^nu} as a torus word
FHE_WOP_HD inline uint64_t wop_table_at(size_t c, int nu, int cb_log_b, int cb_d, int log_delta) {
    return uint64_t(0) - wop_h(int(c & ((size_t(1) << nu) - 1)), cb_log_b, cb_d, log_delta);
}

// the shape checks that need no device: FHE_OK, FHE_ERR_INVALID or FHE_ERR_UNSUPPORTED
inline int wop_check(int cb_log_b, int cb_d, size_t n, int m) {
    if (m < 1 || cb_d < 1 || cb_d > CBS_MAX_D || cb_log_b < 1 || cb_log_b * cb_d > 63 || !cbs_pow2(n)) return FHE_ERR_INVALID;
    // a quarter of the ring holds whole groups of 2^nu coefficients (every admitted ring passes: n / 4 >= 64 >= 2^nu = 32 at most)
    if (n < 4 || (n / 4) % (size_t(1) << wop_nu(cb_d))) return FHE_ERR_INVALID;
    if (m > WOP_MAX_BITS || n < 256 || n > 2048) return FHE_ERR_UNSUPPORTED;
    return FHE_OK;
}

// The test polynomial of the step whose bit stands at log_delta; log_delta < 0: the last step's.  out [n].
inline int wop_table(int cb_log_b, int cb_d, size_t n, int log_delta, uint64_t *out) {
    if (!out || log_delta == 0 || log_delta > 63) return FHE_ERR_INVALID;
    const int rc = wop_check(cb_log_b, cb_d, n, 1);
    if (rc != FHE_OK) return rc;
    const int nu = wop_nu(cb_d);
    for (size_t c = 0; c < n; ++c) out[c] = wop_table_at(c, nu, cb_log_b, cb_d, log_delta);
    return FHE_OK;
}

// the level row of (ciphertext c, bit l, level j) among the batch m cb_d inputs of the private functional key switch: groups of cb_d in
// the order [c][l], the order of fhe_tfhe_lut_eval's selectors
inline size_t wop_level_row(size_t c, int l, int j, int m, int cb_d) { return (c * size_t(m) + size_t(l)) * size_t(cb_d) + size_t(j); }

// Stream-ordered scratch of fhe_tfhe_wop_selectors in 64-bit words.  L (tfhe_circuit.hpp: TfheScratch): the batch blind rotations of ONE
// step, the batch m cb_d level rows of ALL steps, the mod-switched a~, b~.  Behind it, from an even word on: the extracted correction
// rows cx.a [batch][n], the m step tables [m][n], then the running remainder and the correction under the small key, [batch][n_lwe]
// each, and the three b arrays [batch].
struct WopScratch {
    TfheScratch L;
    size_t cx_a, tab, rem_a, cor_a, rem_b, cor_b, cx_b, total;
    WopScratch(size_t n, size_t n_lwe, int m, int cb_d, size_t batch) : L(batch, batch * size_t(m) * size_t(cb_d), n, n_lwe, 0, false) {
        cx_a = (L.total + 1) & ~size_t(1);
        tab = cx_a + batch * n;
        rem_a = tab + size_t(m) * n;
        cor_a = rem_a + batch * n_lwe;
        rem_b = cor_a + batch * n_lwe;
        cor_b = rem_b + batch;
        cx_b = cor_b + batch;
        total = cx_b + batch;
    }
};

// every launch counts rows and jobs in 32 bits
inline int wop_batch_check(int m, int cb_d, size_t n_lwe, size_t batch) {
    const size_t lim = 0x7fffffffull;
    if (batch > lim / (2 * size_t(m) * size_t(cb_d)) || batch > lim / (n_lwe + 1)) return FHE_ERR_UNSUPPORTED;
    return FHE_OK;
}

inline int wop_workspace(size_t n, size_t n_lwe, int m, int cb_d, size_t batch, size_t *words) {
    if (!words || n_lwe == 0) return FHE_ERR_INVALID;
    int rc = wop_check(1, cb_d, n, m);  // the gadget base does not size anything
    if (rc == FHE_OK) rc = wop_batch_check(m, cb_d, n_lwe, batch);
    if (rc != FHE_OK) return rc;
    *words = WopScratch(n, n_lwe, m, cb_d, batch).total;
    return FHE_OK;
}

}  // namespace fhe
