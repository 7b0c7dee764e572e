// Host logic of the packing key switch (fhe_tlwe_pack_key_prepare, fhe_tlwe_pack): plain C++ (no HIP), so that it also builds into a
// stand-alone program.  What is here: the argument checks that need no device, the exactness bound of the two 60-bit primes stated in
// key rows, and the chunk rule -- how the d (n_in + 1) rows of a key are cut into runs that one team sums before its inverse
// transforms.
//
// The pack is a sum of polynomial products, out = sum_rows D_row(X) * key[row] in Z_{2^64}[X]/(X^n + 1), D_row a polynomial of signed
// digits (|digit| <= 2^(log_b - 1)) and the key words read as signed 64-bit integers.  Summed over R rows a coefficient stays below
// R n 2^(62 + log_b) in absolute value; the two primes recover it while that is below p0 p1 / 2 ~ 2^118.9.  The rule asks for
// R n 2^(64 + log_b) < 2^118: torus_kernels.hpp's criterion with R in place of 2d, two bits to spare.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fhe_ring.h"
#include "tfhe_cbs.hpp"  // cbs_gadget_ok, PFKS_MAX_LOG_B

namespace fhe {

constexpr size_t PACK_MIN_ROWS = 8;       // the library's rule cuts no chunk shorter: four inverse transforms (two per prime) and 2n atomic adds per chunk
constexpr size_t PACK_TEAMS_PER_CU = 12;  // teams the rule wants per compute unit: three are resident at n = 1024 (152 VGPRs), four rounds
                                          // of them keep the last round's idle share small (DESIGN.md 9.8 has the sweep)

// the largest R with R n 2^(64 + log_b) < 2^118, n = 2^log_n
inline size_t pack_max_rows(int log_n, int log_b) {
    const int e = 118 - 64 - log_b - log_n;
    if (e <= 0) return 0;
    return e >= 62 ? (size_t(1) << 62) - 1 : (size_t(1) << e) - 1;
}

// the checks of fhe_tlwe_pack_key_prepare that need no device; n must be one of the torus context's rings (2^8 .. 2^11)
inline int pack_key_check(int log_b, int d, size_t n_in, size_t n) {
    if (!cbs_gadget_ok(log_b, d) || n_in == 0) return FHE_ERR_INVALID;
    if (!cbs_pow2(n) || n < 256 || n > 2048) return FHE_ERR_INVALID;
    if (log_b > PFKS_MAX_LOG_B) return FHE_ERR_UNSUPPORTED;
    if (n_in >= (size_t(1) << 31) - 1 || size_t(d) * (n_in + 1) >= (size_t(1) << 31)) return FHE_ERR_UNSUPPORTED;
    return FHE_OK;
}

// the checks of fhe_tlwe_pack on count, stride and the ring
inline int pack_call_check(size_t count, size_t stride, size_t n) {
    if (count < 1 || stride < 1 || count > n) return FHE_ERR_INVALID;
    if (count == 1) return FHE_OK;               // one input lands at coefficient 0 whatever the stride
    if (stride >= n) return FHE_ERR_INVALID;     // (and the product below cannot wrap)
    return (count - 1) * stride < n ? FHE_OK : FHE_ERR_INVALID;
}

// Chunk c of a plan covers the rows c per_chunk .. min(rows, (c + 1) per_chunk) - 1: every row once, no chunk empty, no chunk longer
// than pack_max_rows.
struct PackPlan {
    size_t chunks, per_chunk;
};

// rows = d (n_in + 1) > 0.  forced = the lab switch PACK_SPLIT: k >= 1 asks for k chunks per pack, clamped to [what the bound needs, rows];
// 0 is the library's rule: enough chunks that packs x chunks teams fill the chip (PACK_TEAMS_PER_CU per compute unit), none shorter than
// PACK_MIN_ROWS unless the bound says so.
inline PackPlan pack_plan(size_t rows, int log_n, int log_b, size_t packs, size_t cus, long forced) {
    const size_t cap = pack_max_rows(log_n, log_b);
    if (rows == 0 || cap == 0) return PackPlan{0, 0};
    const size_t need = (rows + cap - 1) / cap;
    size_t chunks;
    if (forced >= 1) chunks = (size_t)forced;
    else {
        const size_t want = PACK_TEAMS_PER_CU * (cus ? cus : 1), p = packs ? packs : 1;
        chunks = (want + p - 1) / p;
        const size_t longest = rows / PACK_MIN_ROWS;
        if (chunks > longest) chunks = longest;
    }
    if (chunks < need) chunks = need;
    if (chunks > rows) chunks = rows;
    if (chunks < 1) chunks = 1;
    const size_t per = (rows + chunks - 1) / chunks;
    return PackPlan{(rows + per - 1) / per, per};
}

// Which product a call runs.  The transforms cost the same whatever `count` is; the scalar digits x key product of fhe_tlwe_pfks followed
// by one rotate-and-add kernel costs `count` times a small unit, and wins while count is small (DESIGN.md 9.8 has the measured crossover).
// forced = the lab switch PACK_ROUTE: 1 the transforms, 2 the scalar product, anything else the rule.  The bits are the same either way.
constexpr size_t PACK_SCALAR_MAX_COUNT = 16;
inline bool pack_scalar_route(size_t count, long forced) { return forced == 2 || (forced != 1 && count <= PACK_SCALAR_MAX_COUNT); }

// packs one launch group works on: what `budget` bytes of scratch hold at `per_pack` bytes each, at least one, at most `cap` (a grid
// dimension) and at most the lab switch PACK_SLAB where that is >= 1
inline size_t pack_slab(size_t packs, size_t per_pack, size_t budget, size_t cap, long forced) {
    size_t s = per_pack ? budget / per_pack : packs;
    if (forced >= 1 && (size_t)forced < s) s = (size_t)forced;
    if (s > cap) s = cap;
    if (s > packs) s = packs;
    return s < 1 ? 1 : s;
}

// bytes of one stored digit: a byte holds [-64, 64] (log_b <= 7; base 2^8 has digits -128 .. 128, one value too many), 16 bits up to
// log_b = 15, 32 bits up to log_b = 31
inline int pack_digit_bytes(int log_b) { return log_b <= 7 ? 1 : (log_b <= 15 ? 2 : 4); }

}  // namespace fhe
