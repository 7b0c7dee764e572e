// Host logic of the encrypted table look-up with vertical packing (fhe_tfhe_lut_shape, _pack, _workspace, _eval): plain C++ (no HIP), so
// that it also builds into a stand-alone program.  What is here: the shape of a look-up, the packing of the plaintext table into
// polynomials, the extraction indices, the workspace and every argument check that needs no device.
//
// A table T[o][x] (o < n_out outputs, x < 2^m addresses) is read under m TGGSW selectors per ciphertext (address bit l = 0 least
// significant).  The low r = min(m, log2 n) bits ROTATE a packed polynomial: acc <- CMUX(selector l; acc, acc X^(-2^l)) brings
// coefficient j + (address mod 2^r) to j.  The h = m - r bits above them pick one of 2^h polynomials through a CMUX tree
// (tggsw.rs:114-121).  When 2^m < n, per_acc = n / 2^m outputs share one accumulator, output u at coefficients u 2^m ..; the value of
// output u is then sample_extract(u 2^m) (tglwe.rs:115-127).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fhe_ring.h"
#include "tfhe_circuit.hpp"  // TfheScratch

namespace fhe {

constexpr int LUT_MAX_TREE_BITS = 10;      // address bits above log2 n: a tree of at most 1024 leaves per accumulator
constexpr size_t LUT_MAX_POLYS = 65536;    // packed polynomials of one table

struct LutShape {
    int log_n = 0, m = 0;
    int r = 0, h = 0;                       // rotation bits, tree bits: r + h = m
    size_t n = 0, n_out = 0;
    size_t per_acc = 0, n_acc = 0, n_polys = 0;  // outputs per accumulator, accumulators G, polynomials G 2^h
};

// FHE_OK and *S filled, FHE_ERR_INVALID (m < 1, n_out < 1, n no power of two) or FHE_ERR_UNSUPPORTED (n outside 256 .. 2048, more than
// LUT_MAX_TREE_BITS tree bits, more than LUT_MAX_POLYS polynomials)
inline int lut_shape(int m, size_t n_out, size_t n, LutShape *S) {
    if (!S || m < 1 || n_out < 1 || !n || (n & (n - 1))) return FHE_ERR_INVALID;
    if (n < 256 || n > 2048) return FHE_ERR_UNSUPPORTED;
    int log_n = 0;
    while ((size_t(1) << log_n) < n) ++log_n;
    const int r = m < log_n ? m : log_n, h = m - r;
    if (h > LUT_MAX_TREE_BITS) return FHE_ERR_UNSUPPORTED;
    const size_t per_acc = m < log_n ? n >> m : 1;
    const size_t n_acc = n_out / per_acc + (n_out % per_acc ? 1 : 0);
    if (n_acc > LUT_MAX_POLYS || (n_acc << h) > LUT_MAX_POLYS) return FHE_ERR_UNSUPPORTED;
    S->log_n = log_n; S->m = m; S->r = r; S->h = h;
    S->n = n; S->n_out = n_out;
    S->per_acc = per_acc; S->n_acc = n_acc; S->n_polys = n_acc << h;
    return FHE_OK;
}

// where table word (o, x) lives: polynomial (g, t) = g 2^h + t, coefficient u 2^m + i
inline size_t lut_poly_of(const LutShape &S, size_t o, size_t x) { return ((o / S.per_acc) << S.h) + (x >> S.r); }
inline size_t lut_coef_of(const LutShape &S, size_t o, size_t x) { return ((o % S.per_acc) << S.m) + (x & ((size_t(1) << S.r) - 1)); }
// the accumulator of output o and the coefficient its value is extracted from (below n: u < per_acc <= n / 2^m)
inline size_t lut_acc_of(const LutShape &S, size_t o) { return o / S.per_acc; }
inline size_t lut_extract_index(const LutShape &S, size_t o) { return (o % S.per_acc) << S.m; }

// table [n_out][2^m] torus words -> polys [n_acc][2^h][n]: every table word once, zero elsewhere
inline int lut_pack(const uint64_t *table, int m, size_t n_out, size_t n, uint64_t *polys) {
    LutShape S;
    const int rc = lut_shape(m, n_out, n, &S);
    if (rc != FHE_OK) return rc;
    if (!table || !polys) return FHE_ERR_INVALID;
    for (size_t i = 0; i < S.n_polys * n; ++i) polys[i] = 0;
    const size_t entries = size_t(1) << m;
    for (size_t o = 0; o < n_out; ++o)
        for (size_t x = 0; x < entries; ++x) polys[lut_poly_of(S, o, x) * n + lut_coef_of(S, o, x)] = table[o * entries + x];
    return FHE_OK;
}

// Tree level v reads 2^(h - v) nodes per accumulator and writes half as many.  A level cannot run in place (the team of pair p writes
// node p while the team of pair p / 2 reads it), so the levels alternate between two areas: X, 2^(h - 1) nodes per accumulator (levels
// 0, 2, ..), and Y behind it, 2^(h - 2) nodes (levels 1, 3, ..).  h = 0: one node, the accumulator the rotation starts from the table.
inline size_t lut_nodes_per_acc(int h) { return h == 0 ? 1 : (size_t(1) << (h - 1)) + (h >= 2 ? size_t(1) << (h - 2) : 0); }
// node offset (in ciphertexts) of the area level v writes, for `accs` = batch n_acc accumulators
inline size_t lut_level_area(int h, int v, size_t accs) { return (v & 1) ? accs << (h - 1) : 0; }
// where the accumulators stand when the tree is done (h = 0: area X)
inline size_t lut_acc_area(int h, size_t accs) { return h == 0 ? 0 : lut_level_area(h, h - 1, accs); }

// the size checks of a call: FHE_OK, or FHE_ERR_UNSUPPORTED when a launch would pass 2^31 - 1 teams or rows
inline int lut_batch_check(const LutShape &S, size_t batch) {
    const size_t lim = 0x7fffffffull;
    if (batch > lim / S.n_out || batch > lim / (S.n_acc * lut_nodes_per_acc(S.h)) || batch > lim / (size_t)S.m) return FHE_ERR_UNSUPPORTED;
    return FHE_OK;
}

// Stream-ordered scratch of fhe_tfhe_lut_eval in 64-bit words (tfhe_circuit.hpp: TfheScratch): the tree's nodes and the accumulators as
// its "blind rotations" (acc.a, acc.b [batch n_acc nodes][n]); with a key switch (n_lwe_out > 0) the batch n_out extracted TLWEs, which
// otherwise go straight to the caller's output.  No mod-switched inputs (n_lwe = 0), no wire table.
inline TfheScratch lut_scratch(const LutShape &S, size_t n_lwe_out, size_t batch) {
    return TfheScratch(batch * S.n_acc * lut_nodes_per_acc(S.h), n_lwe_out ? batch * S.n_out : 0, S.n, 0, 0, false);
}
inline int lut_workspace(size_t n, int m, size_t n_out, size_t n_lwe_out, size_t batch, size_t *words) {
    if (!words) return FHE_ERR_INVALID;
    LutShape S;
    int rc = lut_shape(m, n_out, n, &S);
    if (rc == FHE_OK) rc = lut_batch_check(S, batch);
    if (rc != FHE_OK) return rc;
    *words = lut_scratch(S, n_lwe_out, batch).total;
    return FHE_OK;
}

// the selectors of a call lie inside the prepared key: first_index + batch m <= count, without overflow
inline bool lut_selectors_ok(size_t first_index, size_t batch, int m, size_t count) {
    return first_index <= count && batch <= (count - first_index) / (size_t)m;
}

}  // namespace fhe
