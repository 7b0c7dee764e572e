// csrc/tfhe_pack.hpp alone (no HIP, no library): the exactness bound of the packing key switch in key rows, the chunk rule, the route and
// slab rules and the argument checks.  A stand-alone program (AddressSanitizer + UBSan in tests/test_tfhe_pack_cpu.py); it runs the checks and prints
// "tfhe_pack_host_test ok".
#include <cstdio>
#include <vector>

#include "../learn-fhe_amd/csrc/tfhe_pack.hpp"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

typedef unsigned __int128 u128;

// R n 2^(64 + log_b) < 2^118, restated on 128-bit integers
static bool bound_holds(size_t r, int log_n, int log_b) { return (((u128)r << log_n) << (64 + log_b)) < ((u128)1 << 118); }

// every row once, in order, no chunk empty or above the bound
static int covers(const fhe::PackPlan &p, size_t rows, int log_n, int log_b) {
    CHECK(p.chunks >= 1 && p.per_chunk >= 1);
    std::vector<int> seen(rows, 0);
    for (size_t c = 0; c < p.chunks; ++c) {
        const size_t first = c * p.per_chunk, last = first + p.per_chunk < rows ? first + p.per_chunk : rows;
        CHECK(first < rows && last > first);
        CHECK(bound_holds(last - first, log_n, log_b));
        for (size_t r = first; r < last; ++r) ++seen[r];
    }
    for (size_t r = 0; r < rows; ++r) CHECK(seen[r] == 1);
    return 0;
}

static int checks() {
    using namespace fhe;
    // the bound: the largest R that holds it, and one more does not
    for (int log_n = 8; log_n <= 11; ++log_n)
        for (int log_b = 1; log_b <= 31; ++log_b) {
            const size_t cap = pack_max_rows(log_n, log_b);
            CHECK(cap >= 1 && bound_holds(cap, log_n, log_b) && !bound_holds(cap + 1, log_n, log_b));
        }
    CHECK(pack_max_rows(11, 31) == 4095 && pack_max_rows(10, 7) == (size_t(1) << 37) - 1);
    // the rule and the lab switch over a grid of shapes
    const size_t row_counts[] = {1, 2, 7, 8, 9, 18, 27, 64, 1000, 3155, 4095, 4096, 4097, 5125, 8190, 8191, 20000};
    for (int log_n : {8, 10, 11})
        for (int log_b : {4, 7, 8, 16, 30, 31})
            for (size_t rows : row_counts)
                for (size_t packs : {size_t(1), size_t(3), size_t(16), size_t(1024), size_t(100000)})
                    for (size_t cus : {size_t(1), size_t(256), size_t(304)})
                        for (long forced : {0L, 1L, 2L, 3L, 27L, 1000000L}) {
                            const PackPlan p = pack_plan(rows, log_n, log_b, packs, cus, forced);
                            if (covers(p, rows, log_n, log_b)) return 1;
                            const size_t cap = pack_max_rows(log_n, log_b), need = (rows + cap - 1) / cap;
                            CHECK(p.chunks >= need && p.chunks <= rows);
                            if (forced >= 1) {  // k chunks, clamped to [need, rows]; the even cut may need fewer than asked
                                const size_t k = (size_t)forced < need ? need : ((size_t)forced > rows ? rows : (size_t)forced);
                                CHECK(p.per_chunk == (rows + k - 1) / k && p.chunks <= k);
                            } else {
                                CHECK(p.chunks <= PACK_TEAMS_PER_CU * cus || p.chunks == need);
                                CHECK(p.per_chunk >= PACK_MIN_ROWS || p.chunks == 1 || p.chunks == need);
                            }
                        }
    // named cases: one row per chunk; a whole key in one chunk; the bound cuts (n = 2048, log_b = 31: 4095 rows at most)
    CHECK(pack_plan(27, 8, 7, 1, 256, 27).chunks == 27 && pack_plan(27, 8, 7, 1, 256, 27).per_chunk == 1);
    CHECK(pack_plan(27, 8, 7, 1, 256, 1).chunks == 1 && pack_plan(18, 11, 31, 1, 256, 1).chunks == 1);
    CHECK(pack_plan(4096, 11, 31, 1 << 20, 256, 0).chunks == 2 && pack_plan(4096, 11, 31, 1, 256, 1).chunks == 2);
    CHECK(pack_plan(4096, 11, 31, 1, 256, 1).per_chunk == 2048);
    CHECK(pack_plan(5125, 10, 7, 1, 256, 0).chunks > 256 && pack_plan(5125, 10, 7, 4096, 256, 0).chunks == 1);
    CHECK(pack_plan(0, 10, 7, 1, 256, 0).chunks == 0);
    // the route rule: the scalar product up to PACK_SCALAR_MAX_COUNT inputs a pack, the transforms above; the lab switch forces either
    CHECK(pack_scalar_route(1, 0) && pack_scalar_route(PACK_SCALAR_MAX_COUNT, 0) && !pack_scalar_route(PACK_SCALAR_MAX_COUNT + 1, 0) && !pack_scalar_route(2048, 0));
    CHECK(!pack_scalar_route(1, 1) && pack_scalar_route(2048, 2) && pack_scalar_route(1, -1) && !pack_scalar_route(2048, 7));
    // packs per launch group: what the budget holds, at least one, never above the cap, the packs or the lab switch
    CHECK(pack_slab(16, 100, 1000, 65535, 0) == 10 && pack_slab(16, 100, 10000, 65535, 0) == 16 && pack_slab(16, 2000, 1000, 65535, 0) == 1);
    CHECK(pack_slab(16, 100, 1000, 4, 0) == 4 && pack_slab(16, 100, 1000, 65535, 3) == 3 && pack_slab(16, 100, 1000, 65535, 50) == 10 &&
          pack_slab(2, 100, 1000, 65535, 1) == 1 && pack_slab(1, 0, 1000, 65535, 0) == 1);
    // digit widths
    CHECK(pack_digit_bytes(1) == 1 && pack_digit_bytes(7) == 1 && pack_digit_bytes(8) == 2 && pack_digit_bytes(15) == 2 && pack_digit_bytes(16) == 4 &&
          pack_digit_bytes(31) == 4);
    // argument checks
    CHECK(pack_key_check(7, 3, 8, 256) == FHE_OK && pack_key_check(31, 2, 8, 2048) == FHE_OK && pack_key_check(16, 4, 1024, 1024) == FHE_OK);
    CHECK(pack_key_check(7, 10, 8, 256) == FHE_ERR_INVALID && pack_key_check(33, 2, 8, 256) == FHE_ERR_INVALID);  // log_b d > 64
    CHECK(pack_key_check(32, 2, 8, 256) == FHE_ERR_UNSUPPORTED && pack_key_check(0, 2, 8, 256) == FHE_ERR_INVALID);
    CHECK(pack_key_check(7, 3, 0, 256) == FHE_ERR_INVALID && pack_key_check(7, 3, 8, 128) == FHE_ERR_INVALID && pack_key_check(7, 3, 8, 4096) == FHE_ERR_INVALID &&
          pack_key_check(7, 3, 8, 1000) == FHE_ERR_INVALID);
    CHECK(pack_call_check(1, 1, 256) == FHE_OK && pack_call_check(256, 1, 256) == FHE_OK && pack_call_check(3, 85, 256) == FHE_OK &&
          pack_call_check(1, 256, 256) == FHE_OK && pack_call_check(1, ~size_t(0), 256) == FHE_OK && pack_call_check(16, 17, 256) == FHE_OK);
    CHECK(pack_call_check(0, 1, 256) == FHE_ERR_INVALID && pack_call_check(1, 0, 256) == FHE_ERR_INVALID && pack_call_check(257, 1, 256) == FHE_ERR_INVALID &&
          pack_call_check(4, 86, 256) == FHE_ERR_INVALID && pack_call_check(2, 256, 256) == FHE_ERR_INVALID &&
          pack_call_check(2, ~size_t(0), 256) == FHE_ERR_INVALID && pack_call_check(17, 16, 256) == FHE_ERR_INVALID);
    return 0;
}

int main() {
    if (checks()) return 1;
    std::printf("tfhe_pack_host_test ok\n");
    return 0;
}
